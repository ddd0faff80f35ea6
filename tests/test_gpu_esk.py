"""abn_esk_score, abn_esk_segment and ESKMeans on the MI355X against tests/esk_np.py.

1. Fused == unfused, bit for bit: cand_id / cand_best equal discovery.segment_vectors + kmeans.assign over the explicitly
   built candidate table wherever keep != 0, and are -1 / NaN everywhere else.
2. Scores against the float64 restatement within the fp32 forward bound of tests/kmeans_np.py at depth frames D + 1.
3. The DP on half-integer inputs (every fp32 operation exact, ties plentiful) EQUALS the restatement.
4. The DP on float data stays within esk_np.dp_bound (2 L delta) of the float64 optimum.
5. Planted words are recovered; fit is reproducible; save / load; an empty cluster keeps its centroid."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import esk_np  # noqa: E402

pytestmark = pytest.mark.gpu

# (S, landmarks per utterance): 2, 127, 129, 147 and 294 candidate slots -- one block, one short of / one past a block of
# 128, and three blocks with utterances that straddle the block edges; utterances of 2, 7 and 40 landmarks
LAYOUTS = ((1, (2,)), (1, (40, 40, 40, 7)), (1, (40, 40, 40, 7, 2)), (3, (40, 2, 7)), (6, (2, 40, 7)))
KS = (1, 128, 129, 300)
DEPTHS = ((2, 2), (31, 1), (4, 8), (4, 9), (10, 40), (8, 64))        # frames x D = 4, 31, 32, 36, 400, 512
GAPS = (1, 1, 2, 3, 5, 12)                                          # frames between landmarks: mostly shorter than `frames`


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def corpus(counts, D, seed, special=True):
    """(table [T, D], lm, lm_off): utterances of the given landmark counts laid out in REVERSE order in the table with two
    rows outside every utterance between them; with `special` a NaN row, an infinite value and an all-zero segment."""
    rng = np.random.default_rng(seed)
    gaps = [rng.choice(GAPS, size=n - 1) for n in counts]
    starts, o = [0] * len(counts), 2
    for u in reversed(range(len(counts))):
        starts[u] = o
        o += int(gaps[u].sum()) + 2
    table = rng.standard_normal((o, D)).astype(np.float32)
    lm = np.concatenate([starts[u] + np.concatenate(([0], np.cumsum(gaps[u]))) for u in range(len(counts))]).astype(np.int64)
    lm_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    if special and len(lm) > 30:
        table[lm[3]:lm[4]] = 0.0                                     # candidate (3, 1) is all zero
        table[lm[9], 0] = np.nan
        table[lm[17], D - 1] = np.inf
    return table, lm, lm_off


def tables(K, depth, seed):
    from abnet3_amd import kmeans
    mu = np.random.default_rng(seed).standard_normal((K, depth)) / np.sqrt(depth)
    return kmeans.score_tables(mu)


def unfused(table, lm, lm_off, m, b, frames, S, max_frames):
    """(best [n_lm S], id [n_lm S]) through the candidate table the fused kernel avoids."""
    from abnet3_amd import kmeans
    from abnet3_amd.discovery import segment_vectors
    row0, n = esk_np.candidates(lm, lm_off, S, max_frames)
    valid = np.flatnonzero(n > 0)
    t = dev(table)
    vec, keep = segment_vectors(t, row0[valid], n[valid].astype(np.int32), frames)
    ids, best = kmeans.assign(vec, torch.zeros(vec.shape[1], device='cuda'), dev(m), dev(b), want_best=True)
    keep = host(keep)
    out_best = np.full(len(n), np.nan, dtype=np.float32)
    out_id = np.full(len(n), -1, dtype=np.int32)
    out_best[valid[keep]], out_id[valid[keep]] = host(best)[keep], host(ids)[keep]
    return out_best, out_id, valid, keep


def fused(table, lm, lm_off, m, b, frames, S, max_frames):
    from abnet3_amd import eskmeans
    best, ids = eskmeans.candidate_scores(dev(table), lm, lm_off, dev(m), dev(b), frames, S, max_frames)
    torch.cuda.synchronize()
    return host(best), host(ids)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.int32), b[~nan].view(np.int32))


def check_fused(layout, K, frames, D, max_frames, seed):
    S, counts = layout
    table, lm, lm_off = corpus(counts, D, seed)
    m, b = tables(K, frames * D, seed + 1)
    want_best, want_id, valid, keep = unfused(table, lm, lm_off, m, b, frames, S, max_frames)
    best, ids = fused(table, lm, lm_off, m, b, frames, S, max_frames)
    assert np.array_equal(ids, want_id), np.flatnonzero(ids != want_id)[:10]
    assert same_bits(best, want_best)
    assert np.array_equal(np.isnan(best), ids < 0)
    return ids, valid, keep


# ---- 1: fused == unfused ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,fd', [(K, fd) for K in KS for fd in DEPTHS])
def test_fused_scores_equal_the_unfused_route_bit_for_bit(K, fd):
    layout = LAYOUTS[(KS.index(K) + DEPTHS.index(fd)) % len(LAYOUTS)]
    check_fused(layout, K, fd[0], fd[1], None if DEPTHS.index(fd) % 2 else 15, seed=1000 * K + fd[0] * fd[1])


@pytest.mark.parametrize('layout', LAYOUTS)
def test_every_layout_with_the_special_rows(layout):
    S, counts = layout
    ids, valid, keep = check_fused(layout, 129, 10, 4, 15, seed=7 + S)
    table, lm, lm_off = corpus(counts, 4, 7 + S)
    row0, n = esk_np.candidates(lm, lm_off, S, 15)
    assert (ids[n == 0] == -1).all()
    assert (ids >= 0).sum() >= 1
    if len(lm) > 30:
        assert not keep.all()                                        # the all-zero segment, the NaN row
        assert ids[3 * S] == -1 and ids[9 * S] == -1 and ids[17 * S] == -1
        if S > 1:
            long = np.flatnonzero((esk_np.candidates(lm, lm_off, S, None)[1] > 15) & (np.arange(len(n)) % S > 0))
            assert len(long) and (ids[long] == -1).all()             # the max_frames cut-off


@pytest.mark.parametrize('S', (1, 3, 6))
def test_spans(S):
    check_fused((S, (7, 40, 2, 7)), 5, 10, 4, 20, seed=40 + S)


@pytest.mark.parametrize('fd', ((64, 1), (65, 1), (100, 4), (128, 4)))
def test_frames_on_both_sides_of_the_tabulated_rows(fd):
    """Up to 64 sampled frames the kernel tabulates the sampled rows in LDS, beyond it divides on the fly."""
    check_fused(LAYOUTS[4], 129, fd[0], fd[1], 40, seed=300 + fd[0])


def test_one_frame_segments_repeat_their_row():
    table = np.random.default_rng(3).standard_normal((6, 3)).astype(np.float32)
    lm, lm_off = np.arange(7, dtype=np.int64), np.array([0, 7], dtype=np.int64)
    m, b = tables(4, 15, 5)
    best, ids = fused(table, lm, lm_off, m, b, 5, 2, None)
    want_best, want_id, _, _ = unfused(table, lm, lm_off, m, b, 5, 2, None)
    assert np.array_equal(ids, want_id) and same_bits(best, want_best)
    v = np.tile(table[2], 5).astype(np.float64)
    s = (v / np.sqrt((v * v).sum())) @ m.astype(np.float64).T + b
    assert ids[2 * 2] == int(np.argmax(s)) and abs(best[2 * 2] - s.max()) < 1e-5


# ---- 2: the float64 restatement -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,fd', [(300, (10, 40)), (129, (4, 9)), (128, (8, 64)), (1, (2, 2))])
def test_scores_within_the_forward_bound_of_the_float64_restatement(K, fd):
    frames, D = fd
    S, counts = LAYOUTS[4]
    table, lm, lm_off = corpus(counts, D, 90 + K, special=False)
    m, b = tables(K, frames * D, 91 + K)
    row0, n = esk_np.candidates(lm, lm_off, S, 25)
    V, bad = esk_np.vectors(table, row0, n, frames)
    best64, id64, gap, E = esk_np.score(V, bad, m, b)
    best, ids = fused(table, lm, lm_off, m, b, frames, S, 25)
    good = ~bad
    assert np.array_equal(ids < 0, bad) and good.sum() > 100
    err = np.abs(best[good].astype(np.float64) - best64[good])
    print('max |best - best64| / E = %.3f' % float((err / E[good]).max()))
    assert (err <= E[good]).all()
    clear = good & (gap > 2.0 * E)
    close = float((good & ~clear).sum()) / good.sum()
    print('candidates under the gap: %.4f' % close)
    assert close <= 0.01
    assert np.array_equal(ids[clear], id64[clear])


# ---- 3: the DP on exact inputs ------------------------------------------------------------------------------------------------
def exact_dp_case(counts, S, seed, block=()):
    """Half-integer cand_best, random ids; `block`: utterances with every candidate out of S landmarks in a row at -1."""
    rng = np.random.default_rng(seed)
    lm_off = np.concatenate(([0], np.cumsum(counts))).astype(np.int64)
    order = rng.permutation(len(counts))                             # the utterances' rows in any order
    lm = np.zeros(lm_off[-1], dtype=np.int64)
    o = 0
    for u in order:
        g = np.concatenate(([0], np.cumsum(rng.integers(1, 10, size=counts[u] - 1))))
        lm[lm_off[u]:lm_off[u + 1]] = o + g
        o += int(g[-1]) + 3
    best = (rng.integers(-4, 5, size=len(lm) * S) / 2.0).astype(np.float32)
    ids = rng.integers(0, 50, size=len(lm) * S).astype(np.int32)
    ids[rng.random(len(ids)) < 0.15] = -1
    for u in range(len(counts)):
        lo, hi = int(lm_off[u]), int(lm_off[u + 1])
        if u in block:                                               # S landmarks in a row: every path lands on one of them
            mid = min(lo + (hi - lo) // 2, hi - 2)
            ids[max(lo, mid - S + 1) * S:(mid + 1) * S] = -1
        else:
            ids[np.arange(lo, hi) * S] = np.abs(ids[np.arange(lo, hi) * S])         # s = 1 always open: reachable
    best[ids < 0] = np.nan
    return best, ids, lm, lm_off


def run_dp(best, ids, lm, lm_off, S):
    from abnet3_amd import eskmeans
    out = eskmeans.segment_dp(dev(best), dev(ids, np.int32), lm, lm_off, S)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


@pytest.mark.parametrize('S', (1, 2, 3, 6, 8))
def test_dp_on_exact_inputs_equals_the_restatement(S):
    counts = (300, 2, 7, 65, 66, 2, 40, 129)
    best, ids, lm, lm_off = exact_dp_case(counts, S, seed=20 + S, block=(2, 6))
    want = esk_np.dp(best, ids, lm, lm_off, S)
    got = run_dp(best, ids, lm, lm_off, S)
    for name, a, w in zip(('cut', 'word', 'span', 'objective', 'n_seg'), got, want):
        assert np.array_equal(a, w, equal_nan=True), (name, np.flatnonzero(a != w)[:10])
    cut, word, span, obj, n_seg = got
    assert np.isnan(obj[2]) and n_seg[2] == -1 and not cut[lm_off[2]:lm_off[3]].any()
    assert (span[lm_off[2]:lm_off[3]] == -1).all() and (word[lm_off[2]:lm_off[3]] == -1).all()
    assert n_seg[0] >= 299 // S and cut[0] == 1 and cut[299] == 1 and n_seg[1] == 1
    assert int((span >= 1).sum()) == int(n_seg[n_seg > 0].sum())


def test_dp_without_the_optional_outputs():
    from abnet3_amd import _lib
    best, ids, lm, lm_off = exact_dp_case((7, 40), 3, seed=4)
    want = esk_np.dp(best, ids, lm, lm_off, 3)
    d = [dev(best), dev(ids, np.int32), dev(lm, np.int64), dev(lm_off, np.int64)]
    cut = torch.full((len(lm),), 9, dtype=torch.uint8, device='cuda')
    word = torch.full((len(lm),), 9, dtype=torch.int32, device='cuda')
    span = torch.full((len(lm),), 9, dtype=torch.int32, device='cuda')
    _lib.check(_lib.load().abn_esk_segment(*[_lib.ptr(t) for t in d], 2, len(lm), 3, _lib.ptr(cut), _lib.ptr(word), _lib.ptr(span),
                                           None, None, _lib.stream()), 'abn_esk_segment')
    torch.cuda.synchronize()
    assert np.array_equal(host(cut), want[0]) and np.array_equal(host(word), want[1]) and np.array_equal(host(span), want[2])


# ---- 4: the DP on float data --------------------------------------------------------------------------------------------------
def test_dp_on_float_data_within_the_derived_bound():
    frames, D, K, S = 10, 8, 20, 6
    counts = (150, 40, 7, 2)
    table, lm, lm_off = corpus(counts, D, 61, special=False)
    m, b = tables(K, frames * D, 62)
    row0, n = esk_np.candidates(lm, lm_off, S, 30)
    V, bad = esk_np.vectors(table, row0, n, frames)
    best64, _, _, E = esk_np.score(V, bad, m, b)
    best, ids = fused(table, lm, lm_off, m, b, frames, S, 30)
    _, _, _, obj, n_seg = run_dp(best, ids, lm, lm_off, S)
    for u, cnt in enumerate(counts):
        lo, L = int(lm_off[u]), cnt - 1
        c64 = np.full((L, S), np.inf)
        used = []
        for g in range(L):
            for s in range(1, min(S, L - g) + 1):
                at = (lo + g) * S + s - 1
                if not bad[at]:
                    c64[g, s - 1] = n[at] * (1.0 - 2.0 * best64[at])
                    used.append(at)
        opt = esk_np.optimum_f64(c64, L, S)
        bound = esk_np.dp_bound(n[used], best64[used], E[used], L)
        print('utterance %d: |objective - optimum| = %.3e, bound %.3e' % (u, abs(obj[u] - opt), bound))
        assert n_seg[u] >= 1 and abs(obj[u] - opt) <= bound
        assert bound < 1e-2 * max(1.0, abs(opt))                     # the bound says something


# ---- 5: planted words, the class ----------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def planted():
    """5 templates of 10 .. 20 frames, D = 8, concatenated with noise at 0.01 of the feature scale; landmarks at the true
    boundaries and the words' midpoints; the alignment that names every word."""
    rng = np.random.default_rng(12)
    D, frames = 8, 10
    lens = (10, 13, 16, 18, 20)
    templates = [rng.standard_normal((n, D)).astype(np.float32) for n in lens]
    feats, times, lms, truth, files, on, off, sym = {}, {}, {}, {}, [], [], [], []
    for u in range(6):
        name = 'utt%d' % u
        words = list(rng.permutation(5)) + list(rng.integers(0, 5, size=3))
        x = np.concatenate([templates[w] for w in words])
        feats[name] = (x + 0.01 * rng.standard_normal(x.shape)).astype(np.float32)
        times[name] = 0.0125 + 0.01 * np.arange(len(x))
        bounds = np.concatenate(([0], np.cumsum([lens[w] for w in words])))
        lms[name] = np.unique(np.concatenate((bounds, (bounds[:-1] + bounds[1:]) // 2))).astype(np.int64)
        truth[name] = (bounds, np.array(words))
        for a, e, w in zip(bounds[:-1], bounds[1:], words):
            files.append(name), on.append(times[name][a] - 0.005), off.append(times[name][e - 1] + 0.005), sym.append('w%d' % w)
    init = np.stack([esk_np.vector(t, 0, len(t), frames)[0] for t in templates]).astype(np.float64)
    return dict(feats=feats, times=times, lms=lms, truth=truth, init=init, frames=frames, D=D,
                align=(files, on, off, sym))


def test_the_restatement_recovers_the_planted_words(planted):
    """The CPU half: tests/esk_np.py alone finds every boundary and one cluster per word type at this seed."""
    from abnet3_amd import kmeans
    m, b = kmeans.score_tables(planted['init'])
    for name, x in planted['feats'].items():
        lm = planted['lms'][name]
        off = np.array([0, len(lm)])
        row0, n = esk_np.candidates(lm, off, 6, None)
        V, bad = esk_np.vectors(x, row0, n, planted['frames'])
        best64, id64, _, _ = esk_np.score(V, bad, m, b)
        cut, word, span, obj, n_seg = esk_np.dp(best64.astype(np.float32), id64, lm, off, 6)
        bounds, words = planted['truth'][name]
        assert np.array_equal(lm[cut > 0], bounds) and np.array_equal(word[span >= 1], words)


def test_planted_words_are_recovered_and_fit_stops(planted, tmp_path):
    from abnet3_amd import eskmeans, tde
    q = eskmeans.ESKMeans(5, frames=planted['frames'], max_span=6, n_iter=10).fit(
        planted['feats'], planted['lms'], init=planted['init'], times=planted['times'])
    assert len(q.objective_) == 2 and q.n_segments_ == [48, 48]        # the first segmentation, and it did not change
    seg = q.segment(planted['feats'], planted['lms'], times=planted['times'])
    for name, (bounds, words) in planted['truth'].items():
        begin, end, ids = seg[name]
        assert np.array_equal(begin, bounds[:-1]) and np.array_equal(end, bounds[1:]) and np.array_equal(ids, words)
    align = tde.make_alignment(*planted['align'])
    path = q.write_classes(str(tmp_path / 'planted.classes'))
    scores = tde.TermEvaluator(align).evaluate(path)
    assert scores.ned == 0.0 and scores.n_clusters == 5 and scores.n_tokens == 48 and scores.coverage == 1.0
    bs = tde.boundary_scores(q.boundaries(), align)
    assert bs.f == 1.0 and bs.n_found == bs.n_gold == bs.n_hit == 42


def test_fit_twice_gives_identical_bytes_and_survives_a_save(planted, tmp_path):
    from abnet3_amd import eskmeans
    lms = eskmeans.uniform_landmarks(planted['feats'], 4)
    fits = [eskmeans.ESKMeans(12, frames=planted['frames'], max_span=4, max_frames=30, n_iter=4, seed=3).fit(planted['feats'], lms)
            for _ in range(2)]
    a, b = fits
    assert a.centroids_.tobytes() == b.centroids_.tobytes() and a.objective_ == b.objective_ and a.n_segments_ == b.n_segments_
    assert np.isfinite(a.objective_).all() and a.n_unreachable_ == 0 and len(a.objective_) >= 2
    assert sum(len(c) for c in a.clusters) == a.n_segments_[-1]
    path = str(tmp_path / 'esk.npz')
    a.save(path)
    c = eskmeans.ESKMeans.load(path)
    assert c.whoami() == a.whoami() and c.centroids_.tobytes() == a.centroids_.tobytes() and c.objective_ == a.objective_
    sa, sc = a.segment(planted['feats'], lms), c.segment(planted['feats'], lms)
    for k in sa:
        assert all(np.array_equal(x, y) for x, y in zip(sa[k], sc[k]))
        assert sa[k][0][0] == 0 and sa[k][1][-1] == len(planted['feats'][k]) and np.array_equal(sa[k][0][1:], sa[k][1][:-1])


def test_an_empty_cluster_keeps_its_centroid(planted):
    from abnet3_amd import eskmeans
    far = -planted['init'].sum(axis=0)
    init = np.concatenate((planted['init'], (far / np.sqrt((far * far).sum()))[None]))
    q = eskmeans.ESKMeans(6, frames=planted['frames'], n_iter=3).fit(planted['feats'], planted['lms'], init=init)
    assert q.counts_[5] == 0 and q.n_empty_ == 1 and np.array_equal(q.centroids_[5], init[5])
    assert (q.counts_[:5] > 0).all() and not np.array_equal(q.centroids_[:5], init[:5])
    assert np.abs(q.centroids_[:5] - init[:5]).max() < 0.02             # the words' means: the templates up to the noise
