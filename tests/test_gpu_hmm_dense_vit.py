"""abnz_hmm_dense_viterbi and TransitionHmmPosteriorgram.decode / quantize on the MI355X against tests/hmm_dense_vit_np.py.

Exact inputs: integer frames in [-3, 3], shift 0, A integer in [-2, 2], B = -0.5, c0, li and lt multiples of 1/8 (li in
[-5, 0], lt in [-3, 0]) -- every fp32 operation of the score GEMM and of the recurrence is then exact, ties are plentiful,
and ids, log_prob, n_switch and n_good must EQUAL the restatement's.  Random float data is compared through the float64 log
joint with the allowance hmm_dense_vit_np's docstring derives (2 n_good delta); the sticky matrix must give
abn_hmm_viterbi's log_prob bit for bit."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import gmm_np  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_np  # noqa: E402
import hmm_vit_np  # noqa: E402
from test_gpu_hmm_vit import dev, host, layout, prefilled, recipe, Scores  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT3_SYMBOLS: the entry the dirty-memory test below reaches, and the host query
DIRTY_CASES = ('abnz_hmm_dense_viterbi',)
QUERIES = ('abnz_hmm_dense_viterbi_ws_bytes',)

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
KS = (1, 2, 5, 16, 17, 32, 33, 64, 65, 127, 128)             # every capacity (16, 32, 64, 128) at both edges
DS = (1, 16, 39, 127)


def exact_case(T, K, D, seed):
    """dict(x, A, B, c0, li, lt, s): integer frames and tables in eighths, the float32 scores s exact."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    A = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = (rng.integers(-16, 17, size=K) / 8.0).astype(np.float32)
    li = (-rng.integers(0, 41, size=K) / 8.0).astype(np.float32)
    lt = (-rng.integers(0, 25, size=(K, K)) / 8.0).astype(np.float32)
    x64, A64 = x.astype(np.float64), A.astype(np.float64)
    s64 = x64 @ A64.T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64)
    return dict(x=x, A=A, B=B, c0=c0, li=li, lt=lt, s=s)


def run(c, off, lens, ids=None, shift=None, want_log_prob=True):
    from abnet3_amd import hmm
    D = c['x'].shape[1]
    shift = np.zeros(D, dtype=np.float32) if shift is None else shift
    out = hmm.dense_viterbi(dev(c['x']), off, lens, dev(shift), dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['li']), dev(c['lt']),
                            ids=ids, want_log_prob=want_log_prob)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


def check_exact(c, off, lens, good=None):
    T = c['x'].shape[0]
    good = np.ones(T, dtype=bool) if good is None else good
    ref = dv.viterbi(c['s'], good, off, lens, c['li'], c['lt'])
    got = run(c, off, lens, ids=prefilled(T))
    assert np.array_equal(got[0], ref[0]), np.flatnonzero(got[0] != ref[0])[:10]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].dtype == np.int32
    return got


def inside_rows(T, off, lens):
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    return inside


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_exact_inputs_equal_the_restatement(K, D):
    off, T = layout(LENGTHS)
    c = exact_case(T, K, D, seed=100 * K + D)
    ids, lp, nsw, ng = check_exact(c, off, LENGTHS)
    assert np.array_equal(ng, LENGTHS)
    inside = inside_rows(T, off, LENGTHS)
    assert (ids[~inside] == -7).all() and (ids[inside] >= 0).all() and (ids[inside] < K).all()
    print('K %d D %d: %d frames of the chosen paths with a tied argmax' % (K, D, dv.ties(c['s'], np.ones(T, dtype=bool), off, LENGTHS, c['li'], c['lt'])))
    # the same utterances handed over in another order: the same rows get the same ids
    perm = np.random.default_rng(K + D).permutation(len(LENGTHS))
    ids2, lp2, nsw2, ng2 = run(c, off[perm], np.array(LENGTHS)[perm], ids=prefilled(T))
    assert np.array_equal(ids2, ids) and np.array_equal(lp2, lp[perm]) and np.array_equal(nsw2, nsw[perm])
    assert np.array_equal(ng2, ng[perm])


# ---- 2: BAD frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [5, 65])
def test_bad_frames_with_exact_inputs_equal_the_restatement(K):
    lens = (140, 5, 260, 3, 300)
    off, T = layout(lens)
    c = exact_case(T, K, 15, seed=33 + K)
    bad = np.zeros(T, dtype=bool)
    # first / middle / last; none; rows 127 and 128; all; a run across the first block boundary and one up to the second
    for u, rows in enumerate(([0, 70, 139], [], [127, 128, 200], [0, 1, 2], list(range(120, 135)) + list(range(250, 256)) + [299])):
        bad[off[u] + np.array(rows, dtype=np.int64)] = True
    c['x'][bad] = np.nan
    c['x'][off[2] + 128, 1:] = 0.0                                                    # one NaN entry is enough
    c['x'][off[0]] = np.inf
    got = check_exact(c, off, lens, ~bad)
    inside = inside_rows(T, off, lens)
    assert np.array_equal(got[0] == -1, bad) and (got[0][inside & ~bad] >= 0).all()
    assert got[1][3] == 0.0 and got[2][3] == 0 and got[3][3] == 0
    assert got[3].tolist() == [137, 5, 257, 0, 300 - 22]


# ---- 3: random float data against the float64 optimum ----------------------------------------------------------------------
def random_transitions(K, seed, sticky):
    """init [K], trans [K, K] float32: Dirichlet rows, mixed with the identity by `sticky`."""
    rng = np.random.default_rng(seed)
    init = rng.dirichlet(np.full(K, 2.0))
    trans = (1.0 - sticky) * rng.dirichlet(np.full(K, 2.0), size=K) + sticky * np.eye(K)
    return init.astype(np.float32), np.ascontiguousarray(trans.astype(np.float32))


@pytest.fixture(scope='module')
def float_cases():
    cache = {}

    def get(K):
        if K not in cache:
            rng = np.random.default_rng(K)
            lens = rng.integers(100, 301, size=6)
            x, shift, w, m, v = recipe(K, 40, lens, seed=2000 + K, run_len=7)
            cache[K] = (lens, x, shift, w, Scores(x, shift, w, m, v))
        return cache[K]
    return get


@pytest.mark.parametrize('K', [5, 37, 128])
def test_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K):
    from abnet3_amd import hmm
    lens, x, shift, w, sc = float_cases(K)
    off = np.cumsum(lens) - lens
    assert not sc.bad.any()
    used, totals = 0.0, []
    for sticky in (0.0, 0.9):
        init, trans = random_transitions(K, 7 * K, sticky)
        li, lt = hmm.log_transitions(init, trans)
        c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, li=li, lt=lt)
        ids, lp, nsw, ng = run(c, off, lens, shift=shift)
        lmax = dv.table_max(li, lt)
        assert np.array_equal(ng, lens)
        for u, (o, n) in enumerate(zip(off, lens)):
            sl = slice(o, o + n)
            good = np.ones(n, dtype=bool)
            opt = dv.optimum_f64(sc.s64[sl], good, li, lt)
            allow = 2.0 * n * dv.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax)
            j64 = dv.J(sc.s64[sl], ids[sl], good, li, lt)
            used = max(used, (opt - j64) / allow, abs(lp[u] - opt) / allow)
            assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (the upper side: float64 rounding of the two sums only)
            assert abs(lp[u] - opt) <= allow
            assert nsw[u] == dv.switches(ids[sl])
        totals.append(int(nsw.sum()))
    print('K %d: the largest share of the bar 2 n_good delta used: %.3g; switches at sticky 0 / 0.9: %s' % (K, used, totals))
    assert totals[1] < totals[0]                                             # a heavier diagonal switches less


# ---- 4: the sticky matrix against abn_hmm_viterbi ----------------------------------------------------------------------------
# seeds for which the restatement reports no tie on the sticky tables (picked on the CPU; asserted below)
STICKY_SEEDS = {5: 3005, 37: 3037, 128: 3128}


@pytest.mark.parametrize('K', [5, 37, 128])
@pytest.mark.parametrize('stay', [0.5, 0.9])
def test_sticky_matrix_gives_abn_hmm_viterbi(K, stay):
    from abnet3_amd import hmm
    lens = np.array([1, 2, 127, 128, 129, 300])
    off = np.cumsum(lens) - lens
    x, shift, w, m, v = recipe(K, 40, lens, seed=STICKY_SEEDS[K], run_len=7)
    assert (w.astype(np.float32) > 0).all()
    sc = Scores(x, shift, w, m, v)
    lw, ls, lr = hmm_vit_np.tables(w, stay)
    lt = dv.sticky_log_transitions(ls, lr)
    d = [dev(a) for a in (x, shift, sc.A, sc.B, sc.c0)]
    ref = [host(t) for t in hmm.viterbi(d[0], off, lens, d[1], d[2], d[3], d[4], dev(lw), dev(ls), dev(lr))]
    got = [host(t) for t in hmm.dense_viterbi(d[0], off, lens, d[1], d[2], d[3], d[4], dev(lw), dev(lt))]
    bits = dirty_memory.bits
    assert np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(got[3], ref[3]) and np.array_equal(got[3], lens)
    s32 = gmm_np.scores(sc.xc, sc.bad, sc.A, sc.B, sc.c0, np.float32)
    assert dv.ties(s32, ~sc.bad, off, lens, lw, lt) == 0
    assert np.array_equal(got[0], ref[0]) and np.array_equal(got[2], ref[2])


# ---- 5: consistency with the sum-product kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize('sticky', [0.0, 0.9])
def test_log_prob_is_below_the_sum_product_likelihood(float_cases, sticky):
    from abnet3_amd import hmm
    from test_gpu_hmm import FLOOR, U
    from test_gpu_hmm_dense import delta_dense
    K = 37
    lens, x, shift, w, sc = float_cases(K)
    off = np.cumsum(lens) - lens
    init, trans = random_transitions(K, 7 * K, sticky)
    li, lt = hmm.log_transitions(init, trans)
    c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, li=li, lt=lt)
    ids, lp, nsw, ng = run(c, off, lens, shift=shift)
    _, ll, ng_fb = hmm.dense_forward_backward(dev(x), off, lens, dev(shift), dev(sc.A), dev(sc.B), dev(sc.c0), dev(init), dev(trans), 'filter')
    ll, ng_fb = host(ll), host(ng_fb)
    assert np.array_equal(ng, ng_fb)
    # the sum-product kernel's own bar on loglik (tests/test_gpu_hmm_dense.py): S + 2 x 2^-24 sum |m_t|, S the sum over the
    # good frames of the score bar eps_t = max(2^-22, 4 x yardstick) x scale and delta = (2 K + 21) 2^-24
    s32 = gmm_np.scores(sc.xc, sc.bad, sc.A, sc.B, sc.c0, np.float32)
    yard = (np.abs(s32.astype(np.float64) - sc.s64) / sc.scale).max()
    eps = max(FLOOR, 4.0 * yard) * sc.scale.max(axis=1)
    lmax = dv.table_max(li, lt)
    for u, (o, n) in enumerate(zip(off, lens)):
        sl = slice(o, o + n)
        bar_ll = (eps[sl] + delta_dense(K)).sum() + 2.0 * U * np.abs(sc.s64[sl].max(axis=1)).sum()
        allow = n * dv.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax) + bar_ll
        assert lp[u] <= ll[u] + allow, (u, lp[u], ll[u], allow)
        assert lp[u] > ll[u] - n * np.log(K) - allow                         # (and not absurdly far below: at most K^n paths)


# ---- 6: region reuse, bits -------------------------------------------------------------------------------------------------
def test_more_utterances_than_workgroups_reuse_the_regions():
    n = 600
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 6, size=n)
    off = 1 + 6 * np.arange(n, dtype=np.int64)
    T = 6 * n + 1
    c = exact_case(T, 5, 4, seed=4)
    ids, lp, nsw, ng = check_exact(c, off, lens)
    inside = inside_rows(T, off, lens)
    assert (ids[~inside] == -7).all() and (~inside).sum() >= n and nsw.max() > 0
    again = run(c, off, lens, ids=prefilled(T))
    assert all(np.array_equal(a, b) for a, b in zip((ids, lp, nsw, ng), again)) and again[1].tobytes() == lp.tobytes()
    only = run(c, off, lens, ids=prefilled(T), want_log_prob=False)
    assert np.array_equal(only[0], ids) and only[1] is None and only[2] is None and np.array_equal(only[3], ng)


def test_two_calls_are_bit_identical_and_other_rows_are_untouched():
    from abnet3_amd import hmm
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 400, size=40)
    off, T = layout(lens, gap=3)
    K, D = 100, 40
    x, shift, w, m, v = recipe(K, D, [T], seed=8, run_len=6)
    sc_A, sc_B, _ = gmm_np.tables(w, m, v)
    li, lt = hmm.log_transitions(*random_transitions(K, 8, 0.8))
    c = dict(x=x, A=sc_A, B=sc_B, c0=hmm_np.emission_offsets(m, v), li=li, lt=lt)
    sentinel = torch.arange(T, dtype=torch.int32, device='cuda') - 100000
    a = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    b = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[1].tobytes() == b[1].tobytes()
    inside = inside_rows(T, off, lens)
    assert np.array_equal(a[0][~inside], host(sentinel)[~inside]) and (~inside).sum() >= 3 * 41
    assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()
    # an utterance alone gives the rows it gave among its neighbours
    u = int(np.argmax(lens))
    one = run(dict(c, x=x[off[u]:off[u] + lens[u]]), [0], [lens[u]], shift=shift)
    assert np.array_equal(one[0], a[0][off[u]:off[u] + lens[u]]) and one[1][0] == a[1][u] and one[2][0] == a[2][u]


# ---- 7: straight at the library ------------------------------------------------------------------------------------------------
def raw(c, off, lens, ws_len=None, fill=-7):
    """(ids, log_prob, n_switch, n_good) host arrays of abnz_hmm_dense_viterbi with the per-utterance outputs and the
    workspace from torch.empty, ids from torch.empty filled with `fill` (None: left as torch.empty gave it)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    T, D = c['x'].shape
    K, n = len(c['c0']), len(off)
    d = {k: dev(c[k]) for k in ('x', 'A', 'B', 'c0', 'li', 'lt')}
    shift = dev(np.zeros(D))
    ids = torch.empty(T, dtype=torch.int32, device='cuda')
    if fill is not None:
        ids.fill_(fill)
    lp = torch.empty(n, dtype=torch.float64, device='cuda')
    nsw = torch.empty(n, dtype=torch.int32, device='cuda')
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    need = lib.abnz_hmm_dense_viterbi_ws_bytes(n, max(1, int(np.max(lens))) if ws_len is None else ws_len, K, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    rc = lib.abnz_hmm_dense_viterbi(p(d['x']), T, D, p(off_d), p(len_d), n, p(shift), p(d['A']), p(d['B']), p(d['c0']), p(d['li']),
                                    p(d['lt']), K, p(ids), p(lp), p(nsw), p(ng), p(ws), need, _lib.stream())
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(ids), host(lp), host(nsw), host(ng)


def test_refused_utterances_are_left_untouched_and_their_neighbours_unaffected():
    K, D, T = 5, 13, 400
    c = exact_case(T, K, D, seed=17)
    off = np.array([0, -1, 10, T - 3, 30, 340], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300, 50], dtype=np.int32)      # fine, off < 0, len < 0, past the end, longer than the workspace holds, fine
    ids, lp, nsw, ng = raw(c, off, lens, ws_len=100)
    assert list(ng) == [5, -1, -1, -1, -1, 50] and list(nsw[1:5]) == [-1] * 4 and np.isnan(lp[1:5]).all()
    assert (ids[5:340] == -7).all() and (ids[390:] == -7).all()
    ref = dv.viterbi(c['s'], np.ones(T, dtype=bool), [0, 340], [5, 50], c['li'], c['lt'])
    assert np.array_equal(ids, ref[0]) and np.array_equal(lp[[0, 5]], ref[1]) and np.array_equal(nsw[[0, 5]], ref[2])
    alone = raw(c, [0, 340], [5, 50])
    assert np.array_equal(alone[0], ids) and np.array_equal(alone[1], lp[[0, 5]])


def test_every_next3_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT3_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT3_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS))


@pytest.mark.parametrize('K', [5, 65])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(K):
    """The entry of DIRTY_CASES with ids, the per-utterance outputs and the workspace from torch.empty under the three
    patterns: the same bits (rows outside every utterance keep the pattern), and they are the restatement's."""
    from abnet3_amd import _lib
    lens = np.array([1, 2, 127, 128, 129, 290], dtype=np.int64)              # a gap of two rows behind every utterance but the last
    off = np.array([0, 3, 7, 136, 266, 397], dtype=np.int64)
    T = int(off[-1] + lens[-1])
    c = exact_case(T, K, 40, seed=K)
    bad = np.zeros(T, dtype=bool)
    bad[[8, 140, 263, 266, 400]] = True                                     # BAD frames leave part of their backpointer rows unwritten
    c['x'][bad] = np.nan
    inside = inside_rows(T, off, lens)
    bits = dirty_memory.bits
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                r = raw(c, off, lens, fill=None)
            assert int(count) >= 5 and count.nbytes > T * 4                  # ids, three outputs and the workspace
            word = int.from_bytes(bytes([byte]) * 4, 'little')
            assert (bits(r[0][~inside]).view(np.uint32) == word).all() and (~inside).sum() == 10
            outs[byte] = [r[0][inside]] + list(r[1:])
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs[byte], outs[0x00])), hex(byte)
    ref = dv.viterbi(c['s'], ~bad, off, lens, c['li'], c['lt'])
    assert np.array_equal(outs[0xFF][0], ref[0][inside]) and all(np.array_equal(a, b) for a, b in zip(outs[0xFF][1:], ref[1:]))


# ---- 8: the public layer -----------------------------------------------------------------------------------------------------
def test_decode_and_quantize_of_a_corpus_and_downstream(tmp_path):
    from abnet3_amd import eskmeans, gmm, hmm, kmeans
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=40, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    w = np.maximum(g.weights_, 1e-8)
    sticky = hmm.StickyHmmPosteriorgram(g, 0.8)
    counts = hmm.bigram_counts(sticky.decode(corpus), 8)                     # the data-driven start the module describes
    trans = (counts + 1.0) / (counts + 1.0).sum(axis=1, keepdims=True)
    h = hmm.TransitionHmmPosteriorgram(g, trans, w / w.sum())
    ids = h.decode(corpus)
    assert list(ids) == corpus.names and h.last_log_prob_.shape == (len(corpus.names),)
    assert h.last_log_prob_.dtype == np.float64 and h.last_n_switch_.dtype == np.int32 and h.last_n_good_.dtype == np.int32
    assert h.n_bad_ == 0 and h.last_n_good_.tolist() == [corpus.length[k] for k in corpus.names]
    for i, k in enumerate(corpus.names):
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],) and (ids[k] >= 0).all() and (ids[k] < 8).all()
        assert h.last_n_switch_[i] == dv.switches(ids[k])
    lp = h.last_log_prob_.copy()
    assert all(np.array_equal(a, c) for a, c in zip(h.decode(feats).values(), ids.values()))      # the dict form
    assert np.array_equal(h.last_log_prob_, lp)
    one = corpus.names[0]
    alone = h.decode(dev(feats[one]))                                                              # a table: ONE utterance
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.int32 and np.array_equal(host(alone), ids[one])
    assert h.last_log_prob_.shape == (1,) and h.last_log_prob_[0] == lp[0]
    # downstream: what KMeansQuantizer.segment's ids feed, and the loop the module closes: decoded units -> bigrams -> a model
    seq = kmeans.unit_sequences(ids)
    assert 0.0 < kmeans.bitrate(seq, corpus.total / 100.0) < np.inf
    seg = kmeans.segments(ids)
    assert all(np.array_equal(seg[k][2], seq[k]) and int((seg[k][1] - seg[k][0]).sum()) == corpus.length[k] for k in ids)
    lm = eskmeans.landmarks_from_units(seg, {k: corpus.length[k] for k in corpus.names})
    assert set(lm) == set(corpus.names) and all(lm[k][0] == 0 and lm[k][-1] == corpus.length[k] for k in lm)
    again = hmm.bigram_counts(ids, 8)
    assert again.shape == (8, 8) and again.sum() == corpus.total - len(corpus.names)
    h2 = hmm.TransitionHmmPosteriorgram(g, (again + 1.0) / (again + 1.0).sum(axis=1, keepdims=True), w / w.sum())
    assert set(h2.decode(corpus)) == set(ids)
    quant = h.quantize(corpus)
    assert isinstance(quant, DeviceCorpus) and quant.names == corpus.names and quant.total == corpus.total
    flat = np.concatenate([ids[k] for k in corpus.names])
    for k in corpus.names:
        assert quant.length[k] == corpus.length[k] and quant.offset[k] == corpus.offset[k]
        assert np.array_equal(quant.times[k], corpus.times[k])
    assert np.array_equal(host(quant.table), g.means_.astype(np.float32)[flat])
    # a BAD frame: id -1 and a row of zeros
    broken = {k: v.copy() for k, v in feats.items()}
    broken[one][2, 1] = np.nan
    bids = h.decode(broken)
    assert bids[one][2] == -1 and (np.delete(bids[one], 2) >= 0).all() and h.n_bad_ == 1
    assert not host(h.quantize(DeviceCorpus(broken, times)).table)[corpus.offset[one] + 2].any()
    # save / load, and the command line
    path = str(tmp_path / 'dense.npz')
    h.save(path)
    loaded = hmm.TransitionHmmPosteriorgram.load(path).decode(corpus)
    assert all(np.array_equal(loaded[k], ids[k]) for k in ids)
    fpath, opath = str(tmp_path / 'feats.npz'), str(tmp_path / 'ids.npz')
    np.savez(fpath, **feats)
    assert hmm.main(['decode', path, fpath, opath]) == 0
    with np.load(opath) as z:
        assert sorted(z.files) == sorted(ids) and all(np.array_equal(z[k], ids[k]) and z[k].dtype == np.int32 for k in ids)
