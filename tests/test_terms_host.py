"""Term discovery without a GPU: the numpy restatement (tests/terms_np.py) against a plain triple loop written from the
definition, its properties, planted copies, the exclusion band, the windowing, the clustering, the written files, and
that the header and the binding carry the new symbols."""
import os
import random
import re
import sys

import numpy as np
import pytest

from conftest import ROOT

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_kl_np  # noqa: E402
import terms_np  # noqa: E402


def plain_local(d, theta):
    """The definition, cell by cell: (score, path_len, start1, start2, end1, end2)."""
    n, m = d.shape
    theta = np.float64(np.float32(theta))
    dead = (0.0, 0, -1, -1)
    cell = {}
    top = (0.0, 0, -1, -1, -1, -1)
    for i in range(n):
        for j in range(m):
            s = theta - np.float64(d[i, j])
            best = dead
            for pi, pj in ((i - 1, j - 1), (i - 1, j), (i, j - 1)):        # diag, up, left
                c = cell.get((pi, pj), dead)
                if (pi, pj) == (i - 1, j - 1) or c[0] > best[0]:
                    best = c
            if best[0] > 0:
                h, ln, si, sj = best[0] + s, best[1] + 1, best[2], best[3]
            else:
                h, ln, si, sj = s, 1, i, j
            cell[(i, j)] = (h, ln, si, sj) if h > 0 else dead
            if cell[(i, j)][0] > top[0]:                                    # row-major: ties stay with the smallest i, then j
                top = cell[(i, j)] + (i, j)
    return (float(top[0]),) + tuple(int(v) for v in top[1:])


def random_cells(rng, trial):
    n, m = int(rng.integers(1, 14)), int(rng.integers(1, 14))
    if trial % 2:
        d = rng.integers(0, 5, (n, m)).astype(np.float32) / np.float32(4)          # many exact ties in H
    else:
        d = rng.random((n, m)).astype(np.float32)
    if trial % 5 == 0:
        d[rng.integers(0, n), rng.integers(0, m)] = np.inf                          # a blocked cell
    return d.astype(np.float64)


def test_the_restatement_equals_a_plain_triple_loop():
    rng = np.random.default_rng(0)
    live = 0
    for trial in range(48):
        d = random_cells(rng, trial)
        for theta in (0.3, 0.5):
            got, ref = terms_np.local_align(d, theta), plain_local(d, theta)
            assert got == ref, (trial, theta)
            live += got[1] > 1
    assert live >= 48
    assert terms_np.local_align(np.full((3, 4), 0.75), 0.5) == (0.0, 0, -1, -1, -1, -1)          # no live cell
    assert terms_np.local_align(np.zeros((0, 4)), 0.5) == (0.0, 0, -1, -1, -1, -1)
    assert terms_np.local_align(np.zeros((4, 0)), 0.5) == (0.0, 0, -1, -1, -1, -1)
    # exact ties: every cell of the diagonal of equal frames is a maximum only at its end; the first row and column win
    assert terms_np.local_align(np.array([[0.0, 1.0], [1.0, 1.0], [0.0, 1.0]]), 0.5) == (0.5, 1, 0, 0, 0, 0)
    assert terms_np.local_align(np.array([[1.0, 0.0], [0.0, 1.0]]), 0.5) == (0.5, 1, 0, 1, 0, 1)


def test_properties_of_a_result():
    rng = np.random.default_rng(1)
    swapped = 0
    for trial in range(40):
        d = rng.random((int(rng.integers(2, 30)), int(rng.integers(2, 30)))).astype(np.float32).astype(np.float64)
        sc, ln, s1, s2, e1, e2 = terms_np.local_align(d, 0.45)
        assert sc >= 0
        if ln == 0:
            continue
        assert 0 <= s1 <= e1 < d.shape[0] and 0 <= s2 <= e2 < d.shape[1]
        span1, span2 = e1 - s1 + 1, e2 - s2 + 1
        assert max(span1, span2) <= ln <= span1 + span2 - 1
        # swapping the sides of a tie-free pair (random cells) swaps the bounds and keeps the score -- up to the order
        # of the float64 additions along the same path, which is the same order: bit-equal
        t = terms_np.local_align(d.T.copy(), 0.45)
        assert t == (sc, ln, s2, s1, e2, e1), trial
        swapped += 1
    assert swapped >= 30


def self_exact(frames):
    """Which frames are at cosine distance exactly 0 from themselves (by value or by the rounding rule)."""
    return np.array([terms_np.cosine_cells(f[None], f[None])[0, 0] == 0 for f in frames])


def test_a_planted_copy_is_found_with_exact_bounds():
    rng = np.random.default_rng(2)
    D, theta = 40, 0.05
    x, y = rng.standard_normal((90, D)).astype(np.float32), rng.standard_normal((120, D)).astype(np.float32)
    # unrelated Gaussian frames sit near distance 0.5 (their cosine has standard deviation 1 / sqrt(40) = 0.16; a distance
    # of 0.2 is a cosine of 0.81, five of them): no cell pays, no extension pays
    d = terms_np.cosine_cells(x, y)
    assert 0.2 < d.min() and d.max() < 0.8 and abs(d.mean() - 0.5) < 0.01
    assert terms_np.local_align(d, theta) == (0.0, 0, -1, -1, -1, -1)
    # the copy: frames whose distance from themselves is exactly 0 (a Gaussian frame's own cosine may round to 1 - 2^-24,
    # distance 1.1e-4; the pool is filtered so that "mean distance 0" is exact)
    pool = rng.standard_normal((400, D)).astype(np.float32)
    word = pool[self_exact(pool)][:37]
    assert len(word) == 37
    x[20:57], y[70:107] = word, word
    sc, ln, s1, s2, e1, e2 = terms_np.local_align(terms_np.cosine_cells(x, y), theta)
    assert (ln, s1, s2, e1, e2) == (37, 20, 70, 56, 106)
    assert sc == 37 * np.float64(np.float32(theta))
    assert np.float64(np.float32(theta)) - sc / ln == 0.0
    # KL: identical posteriorgram rows are at distance exactly 0
    post = rng.dirichlet(np.ones(12), 80).astype(np.float32)
    post[50:62] = post[10:22]
    t = abx_kl_np.tables(post)
    sl = lambda a, b: [v[a:b] for v in t]
    assert terms_np.local_align(terms_np.kl_cells(sl(0, 40), sl(40, 80)), 0.05)[1:] == (12, 10, 10, 21, 21)


def test_exclude_removes_the_self_match_and_finds_the_second_copy():
    rng = np.random.default_rng(3)
    D, theta = 40, 0.05
    utt = rng.standard_normal((160, D)).astype(np.float32)
    pool = rng.standard_normal((300, D)).astype(np.float32)
    word = pool[self_exact(pool)][:25]
    utt[100:125] = word
    utt[30:55] = word
    d = terms_np.cosine_cells(utt, utt)
    sc, ln, s1, s2, e1, e2 = terms_np.local_align(d, theta)
    assert (ln, s1, s2, e1, e2) == (160, 0, 0, 159, 159)                      # the whole diagonal
    sc, ln, s1, s2, e1, e2 = terms_np.local_align(terms_np.exclude_cells(d, 0, 0, 20), theta)
    # the copy at rows 30..54 against columns 100..124: the smallest end row among the two mirror images
    assert (ln, s1, s2, e1, e2) == (25, 30, 100, 54, 124) and sc == 25 * np.float64(np.float32(theta))
    # table rows: the band follows the offsets of the two stretches
    sub = terms_np.exclude_cells(d[:, 90:], 1000, 1090, 20)
    assert np.isinf(sub[95, 5]) and np.isinf(sub[100, 29]) and np.isfinite(sub[100, 30]) and np.isfinite(sub[30, 10])
    assert terms_np.local_align(sub, theta)[1:] == (25, 30, 10, 54, 34)
    assert np.array_equal(terms_np.exclude_cells(d, 5, 5, 0), d)


def test_windows_cover_side_two_and_the_last_is_flush():
    from abnet3_amd import terms
    for window in (1, 2, 7, 64, 512):
        for n in list(range(0, 40)) + [window - 1, window, window + 1, 2 * window, 2 * window + 1, 3 * window + window // 2, 1700]:
            w = terms_np.windows(n, window)
            assert w == terms.windows(n, window)
            if n <= 0:
                assert w == []
                continue
            covered = np.zeros(n, bool)
            for s, k in w:
                assert 0 <= s and s + k <= n and 1 <= k <= window
                covered[s:s + k] = True
            assert covered.all(), (n, window)
            assert w[-1][0] + w[-1][1] == n and w[0][0] == 0
            assert [s for s, _ in w] == sorted({s for s, _ in w})
            if n > window:
                assert all(k == window for _, k in w)
                assert all(b - a <= max(1, window // 2) for (a, _), (b, _) in zip(w, w[1:]))
    assert terms_np.windows(700, 512) == [(0, 512), (188, 512)]
    assert terms_np.kernel_pairs([3, 0, 9], [(0, 0), (0, 1), (1, 2), (0, 2), (2, 2)], 4) == [
        (0, 0, 0, 3), (0, 2, 0, 4), (0, 2, 2, 4), (0, 2, 4, 4), (0, 2, 5, 4), (2, 2, 0, 4), (2, 2, 2, 4), (2, 2, 4, 4), (2, 2, 5, 4)]
    assert terms.kernel_pairs([3, 0, 9], [(0, 2)], 4) == terms_np.kernel_pairs([3, 0, 9], [(0, 2)], 4)


def M(f1, a1, b1, f2, a2, b2, score=1.0):
    from abnet3_amd.terms import Match
    return Match(f1, a1, b1, f2, a2, b2, score, max(b1 - a1, b2 - a2) + 1, 0.01)


def test_clustering_by_union_find():
    from abnet3_amd.terms import cluster_matches
    matches = [
        M(0, 10, 59, 1, 100, 149, 3.0),            # the match join: A = {0:10-59, 1:100-149}
        M(1, 120, 175, 2, 0, 55, 2.0),             # 1:120-175 meets 1:100-149 in 30 of 50 frames: joined to A (a chain)
        M(2, 300, 360, 3, 5, 65, 2.5),             # B = {2:300-360, 3:5-65}
        M(3, 40, 99, 3, 200, 259, 1.0),            # 3:40-99 meets 3:5-65 in 26 of 60 frames: below 0.5, its own cluster C
        M(4, 0, 49, 4, 10, 59, 4.0),               # two fragments of one file that overlap: collapse to one token, dropped
        M(0, 12, 61, 2, 2, 57, 5.0),               # joined to A through 0:10-59 and 2:0-55; higher score: its fragments win
    ]
    got = cluster_matches(matches, 0.5)
    assert got == terms_np.cluster(matches, 0.5)
    assert got == [
        [(0, 12, 61), (1, 100, 149), (2, 2, 57)],   # A: 0:10-59 and 2:0-55 collapsed into the better ones, 1:120-175 into 1:100-149
        [(2, 300, 360), (3, 5, 65)],                # B
        [(3, 40, 99), (3, 200, 259)],               # C: two tokens of one file that do not overlap
    ]
    # a lower threshold joins B and C; 3:40-99 then gives way to 3:5-65 (higher score)
    assert cluster_matches(matches, 0.4)[1] == [(2, 300, 360), (3, 5, 65), (3, 200, 259)]
    assert cluster_matches([], 0.5) == []
    # random matches: the module and the restatement agree, tokens of a cluster's file never overlap, order is defined
    rng = np.random.default_rng(5)
    for trial in range(20):
        ms = []
        for _ in range(int(rng.integers(1, 25))):
            a, b = int(rng.integers(0, 150)), int(rng.integers(0, 150))
            ms.append(M(int(rng.integers(0, 4)), a, a + int(rng.integers(5, 40)), int(rng.integers(0, 4)), b,
                        b + int(rng.integers(5, 40)), float(rng.integers(1, 6))))
        got = cluster_matches(ms, 0.5)
        assert got == terms_np.cluster(ms, 0.5)
        assert got == sorted(got) and all(c == sorted(c) and len(c) >= 2 for c in got)
        for c in got:
            for k, (f, lo, hi) in enumerate(c):
                assert not any(g == f and min(hi, h2) >= max(lo, l2) for g, l2, h2 in c[k + 1:])
        assert cluster_matches(ms[::-1], 0.5) == got or len({m.score for m in ms}) < len(ms)


def test_matches_are_filtered_and_repeats_left_out():
    from abnet3_amd.terms import keep_matches
    kp = [(0, 1, 0, 100), (0, 1, 50, 100), (0, 2, 0, 80), (1, 2, 0, 80), (2, 2, 0, 80), (0, 3, 0, 10)]
    th = np.float64(np.float32(0.05))
    res = (np.array([60 * th, 60 * th, 2.0, 1.0, 0.0, 3.0]), np.array([60, 60, 70, 60, 0, 60], np.int32),
           np.array([5, 5, 0, 0, -1, 0], np.int32), np.array([70, 20, 0, 0, -1, 0], np.int32),
           np.array([64, 64, 59, 59, -1, 59], np.int32), np.array([129 - 0, 79, 48, 59, -1, 59], np.int32))
    got = keep_matches(kp, res, 0.05, 50)
    assert [tuple(m) for m in got] == terms_np.keep_matches(kp, res, 0.05, 50)
    # pair 1 repeats pair 0 (window 50 + 20 = 70); pair 2's side 2 has 49 frames; pair 4 found nothing
    assert [tuple(m)[:6] for m in got] == [(0, 5, 64, 1, 70, 129), (1, 0, 59, 2, 0, 59), (0, 0, 59, 3, 0, 59)]
    assert got[0].distance == 0.0 and got[0].path_len == 60
    assert [tuple(m)[:6] for m in keep_matches(kp, res, 0.05, 50, max_distance=0.02)] == [(0, 5, 64, 1, 70, 129), (0, 0, 59, 3, 0, 59)]


def test_written_files_are_read_back_and_reproducible(tmp_path):
    from abnet3_amd import terms
    from abnet3_amd.dataloader import PairsDataLoader
    from abnet3_amd.sampler import SamplerCluster
    names = ['a', b'b', 'c']
    times = {k: (np.arange(400) + 0.5) * 0.01 + 0.0025 for k in names}
    matches = [M(0, 10, 59, 1, 100, 149, 3.0), M(1, 300, 360, 2, 5, 65, 2.5), M(0, 12, 61, 2, 200, 257, 5.0)]
    clusters = terms.cluster_matches(matches)
    assert clusters == [[(0, 12, 61), (1, 100, 149), (2, 200, 257)], [(1, 300, 360), (2, 5, 65)]]
    out = []
    for d in ('one', 'two'):
        os.makedirs(str(tmp_path / d))
        c = terms.write_classes(str(tmp_path / d / 'terms.classes'), names, times, clusters)
        p, m = terms.write_term_pairs(str(tmp_path / d), names, matches)
        out.append([open(f, 'rb').read() for f in (c, p, m)])
    assert out[0] == out[1]
    assert out[0][0].decode() == terms_np.classes_text(names, times, clusters)
    assert out[0][1].decode() == terms_np.pairs_text([tuple(x) for x in matches])
    assert out[0][2].decode() == terms_np.map_text(names) == '0 a\n1 b\n2 c\n'
    # the .classes file: the sampler's parser gives the same clusters, and its times select exactly the tokens' frames
    parsed = SamplerCluster().parse_input_file(str(tmp_path / 'one' / 'terms.classes'))
    assert len(parsed) == 2 and [len(c) for c in parsed] == [3, 2]
    text = ['a', 'b', 'c']
    for got, want in zip(parsed, clusters):
        for (f, on, off), (g, lo, hi) in zip(got, want):
            assert f == text[g]
            t = times[names[g]]
            assert np.flatnonzero((t >= on) & (t <= off)).tolist() == list(range(lo, hi + 1))
    # the pairs file: the pairs reader takes it (ends exclusive)
    random.seed(0)
    dl = PairsDataLoader(c, None, m, split_method='files')
    dl.pairs_path = p
    dl.load_pairs()
    assert dl.files == {'a', 'b', 'c'}
    lines = out[0][1].decode().splitlines()
    assert lines[0] == '0 1 10 60 100 150 0.01000000000' and len(lines) == 3


def test_header_and_binding_carry_the_new_symbols():
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    for name in ('abn_dtw_local_max_n2', 'abn_dtw_local_batched', 'abn_dtw_local_kl_batched'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SYMBOLS, name
    assert len(_lib.SYMBOLS['abn_dtw_local_batched'][1]) == 19 and len(_lib.SYMBOLS['abn_dtw_local_kl_batched'][1]) == 23
    assert re.search(r'^#define ABN_DTW_LOCAL_MAX_N2 %d$' % terms_np.CAP, text, flags=re.M) and terms_np.CAP >= 512
    assert re.search(r'^#define ABN_ABI_VERSION 20$', text, flags=re.M) and _lib.ABI_VERSION == 20
    from abnet3_amd import build
    assert 'local.hip' in build.SOURCES and build.STRICT_FP['local.hip'] == ['-ffp-contract=off']
    # the library: the cap, and argument validation before any launch
    lib = _lib.load()
    assert lib.abn_dtw_local_max_n2() == terms_np.CAP
    args = [None, 1, None, 1, None, None, None, None, 1, 4]
    out = [None] * 6 + [None]
    assert lib.abn_dtw_local_batched(*(args + [0.5, 0] + out)) == _lib.E_ARG and b'null' in lib.abn_last_error()
    assert lib.abn_dtw_local_batched(*(args + [0.0, 0] + out)) == _lib.E_ARG and b'theta' in lib.abn_last_error()
    assert lib.abn_dtw_local_batched(*(args + [float('inf'), 0] + out)) == _lib.E_ARG and b'theta' in lib.abn_last_error()
    assert lib.abn_dtw_local_batched(*(args + [0.5, -1] + out)) == _lib.E_ARG and b'exclude' in lib.abn_last_error()
    two = [0x1000, 8, 0x2000, 8] + args[4:]
    assert lib.abn_dtw_local_batched(*(two + [0.5, 3] + out)) == _lib.E_ARG and b'one table' in lib.abn_last_error()
    kl = [0x1000, 0x3000, 8, 0x1000, 0x4000, 8, None, None, None, None, 1, 4, 0x5000, 0x5000]
    assert lib.abn_dtw_local_kl_batched(*(kl + [0.5, 3] + out)) == _lib.E_ARG and b'one table' in lib.abn_last_error()


def test_argument_errors_without_a_device(capsys):
    from abnet3_amd import terms
    with pytest.raises(ValueError, match='distance'):
        terms.local_dtw_batch(None, [], [], None, [], [], 0.5, distance='nonsense')
    with pytest.raises(ValueError, match='theta'):
        terms.local_dtw_batch(None, [], [], None, [], [], 0.0)
    with pytest.raises(ValueError, match='theta'):
        terms.local_dtw_batch(None, [], [], None, [], [], float('nan'))
    with pytest.raises(ValueError, match='exclude'):
        terms.local_dtw_batch(None, [], [], None, [], [], 0.5, exclude=-1)
    with pytest.raises(ValueError, match='distance'):
        terms.TermDiscoverer({}, {}, distance='nonsense')
    with pytest.raises(ValueError, match='theta'):
        terms.TermDiscoverer({}, {}, theta=-1.0)
    with pytest.raises(SystemExit):
        terms.main(['feats.h5f', 'out', '--distance', 'euclidean'])
    assert 'kl' in capsys.readouterr().err


def test_the_end_to_end_fixture_is_fair():
    """The restatement finds every planted word of the GPU test's corpus as one cluster holding all its occurrences,
    with exact bounds, and at least one utterance needs two windows."""
    feats, times, planted = terms_np.planted_corpus()
    names = sorted(feats)
    assert max(len(v) for v in feats.values()) > terms_np.CAP and 150 <= min(len(v) for v in feats.values())
    matches, clusters = terms_np.discover(names, feats, 0.05)
    want = sorted(sorted((names.index(k), lo, hi) for k, lo, hi in occ) for occ in planted.values())
    assert clusters == want
    assert all(m[8] < 2e-4 and m[7] == m[2] - m[1] + 1 == m[5] - m[4] + 1 for m in matches)
