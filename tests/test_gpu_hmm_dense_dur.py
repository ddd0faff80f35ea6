"""abnw_hmm_dense_viterbi_dur and TransitionHmmPosteriorgram.decode / quantize with min_duration on the MI355X against
tests/hmm_dense_dur_np.py.

Exact inputs are tests/test_gpu_hmm_dense_vit.py's (`exact_case`: integer frames, tables in eighths): every fp32 operation of
the score GEMM and of the recurrence is then exact, ties are plentiful, and ids, log_prob, n_switch and n_good must EQUAL the
restatement's.  Random float data is compared through the float64 score with the allowance hmm_dense_dur_np's docstring derives
(2 n_good delta); min_duration = 1 must give abnz_hmm_dense_viterbi's bits, and a sticky matrix whose optimum never re-enters a
unit abnx_hmm_viterbi_dur's log_prob."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import hmm_dense_dur_np as dd  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import vit_dur_np  # noqa: E402
from test_gpu_hmm_vit import dev, host, layout, prefilled, recipe, Scores  # noqa: E402
from test_gpu_hmm_dense_vit import exact_case, inside_rows, random_transitions  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT4_SYMBOLS: the entry the dirty-memory test below reaches, and the host query
DIRTY_CASES = ('abnw_hmm_dense_viterbi_dur',)
QUERIES = ('abnw_hmm_dense_viterbi_dur_ws_bytes',)

KS = (1, 2, 5, 16, 17, 33, 64, 65, 127, 128)                  # every capacity (16, 32, 64, 128), at both edges
SS = (2, 3, 8)                                                # every register capacity of the chain (2, 4, 8)
bits = dirty_memory.bits


def lengths_for(S):
    return (0, 1, 2, S - 1, S, S + 1, 63, 64, 65, 127, 128, 129, 300)


def run(c, off, lens, S, ids=None, shift=None, want_log_prob=True):
    from abnet3_amd import hmm
    D = c['x'].shape[1]
    shift = np.zeros(D, dtype=np.float32) if shift is None else shift
    out = hmm.dense_viterbi(dev(c['x']), off, lens, dev(shift), dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['li']), dev(c['lt']),
                            ids=ids, want_log_prob=want_log_prob, min_duration=S)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


def raw(c, off, lens, S, ws_len=None, fill=-7, shift=None):
    """(ids, log_prob, n_switch, n_good) host arrays of abnw_hmm_dense_viterbi_dur with the per-utterance outputs and the
    workspace from torch.empty, ids from torch.empty filled with `fill` (None: left as torch.empty gave it)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    T, D = c['x'].shape
    K, n = len(c['c0']), len(off)
    d = {k: dev(c[k]) for k in ('x', 'A', 'B', 'c0', 'li', 'lt')}
    shift = dev(np.zeros(D) if shift is None else shift)
    ids = torch.empty(T, dtype=torch.int32, device='cuda')
    if fill is not None:
        ids.fill_(fill)
    lp = torch.empty(n, dtype=torch.float64, device='cuda')
    nsw = torch.empty(n, dtype=torch.int32, device='cuda')
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    need = lib.abnw_hmm_dense_viterbi_dur_ws_bytes(n, max(1, int(np.max(lens))) if ws_len is None else ws_len, K, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    rc = lib.abnw_hmm_dense_viterbi_dur(p(d['x']), T, D, p(off_d), p(len_d), n, p(shift), p(d['A']), p(d['B']), p(d['c0']), p(d['li']),
                                        p(d['lt']), K, p(ids), p(lp), p(nsw), p(ng), p(ws), need, _lib.stream(), S)
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(ids), host(lp), host(nsw), host(ng)


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def check_exact(c, off, lens, S, good=None):
    T = c['x'].shape[0]
    good = np.ones(T, dtype=bool) if good is None else good
    ref = dd.viterbi(c['s'], good, off, lens, c['li'], c['lt'], S)
    got = run(c, off, lens, S, ids=prefilled(T))
    assert np.array_equal(got[0], ref[0]), np.flatnonzero(got[0] != ref[0])[:10]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].dtype == np.int32
    for o, n in zip(off, lens):
        assert dd.run_lengths_ok(got[0][o:o + n], S)
    return got


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,S,D', [(K, S, D) for K in KS for S in SS for D in (1, 39)])
def test_exact_inputs_equal_the_restatement(K, S, D):
    lens = lengths_for(S)
    off, T = layout(lens)
    c = exact_case(T, K, D, seed=1000 * K + 10 * D + S)
    ids, lp, nsw, ng = check_exact(c, off, lens, S)
    assert np.array_equal(ng, lens)
    inside = inside_rows(T, off, lens)
    assert (ids[~inside] == -7).all() and (ids[inside] >= 0).all() and (ids[inside] < K).all()
    assert all(nsw[u] == max(len(dd.runs(ids[o:o + n])) - 1, 0) for u, (o, n) in enumerate(zip(off, lens)))
    assert K == 1 or nsw.sum() > 0
    # the same utterances handed over in another order: the same rows get the same ids
    perm = np.random.default_rng(K + D + S).permutation(len(lens))
    ids2, lp2, nsw2, ng2 = run(c, off[perm], np.array(lens)[perm], S, ids=prefilled(T))
    assert np.array_equal(ids2, ids) and np.array_equal(lp2, lp[perm]) and np.array_equal(nsw2, nsw[perm])
    assert np.array_equal(ng2, ng[perm])


# ---- 2: BAD frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,S', [(K, S) for K in (5, 17, 33, 65) for S in (2, 8)])      # every capacity: 16, 32, 64, 128
def test_bad_frames_with_exact_inputs_equal_the_restatement(K, S):
    lens = (140, 5, 300, 3, 300, 90)
    off, T = layout(lens)
    c = exact_case(T, K, 15, seed=33 + K + S)
    bad = np.zeros(T, dtype=bool)
    # first / middle / last; none; rows 127 and 128; all; a run across the first block boundary, one up to the second and the
    # last row; single BAD frames every few rows (inside forced advances) and a run longer than S
    for u, rows in enumerate(([0, 70, 139], [], [127, 128, 200], [0, 1, 2], list(range(120, 135)) + list(range(250, 256)) + [299],
                              list(range(3, 40, 4)) + list(range(50, 50 + S + 3)))):
        bad[off[u] + np.array(rows, dtype=np.int64)] = True
    c['x'][bad] = np.nan
    c['x'][off[2] + 128, 1:] = 0.0                                                    # one NaN entry is enough
    c['x'][off[0]] = np.inf
    got = check_exact(c, off, lens, S, ~bad)
    inside = inside_rows(T, off, lens)
    assert np.array_equal(got[0] == -1, bad) and (got[0][inside & ~bad] >= 0).all()
    assert got[1][3] == 0.0 and got[2][3] == 0 and got[3][3] == 0
    assert got[3].tolist() == [137, 5, 297, 0, 300 - 22, 90 - 10 - (S + 3)]
    # a BAD frame did fall inside a forced advance: it splits a run's first S good frames (read from the restatement's ids)
    ref = dd.viterbi(c['s'], ~bad, off, lens, c['li'], c['lt'], S)[0]
    inside_advance = 0
    for u, (o, n) in enumerate(zip(off, lens)):
        row = ref[o:o + n]
        for r in np.flatnonzero(row == -1):
            before = row[:r][row[:r] >= 0]
            after = row[r + 1:][row[r + 1:] >= 0]
            if len(before) and len(after) and before[-1] == after[0]:
                run_len = 1
                while run_len < len(before) and before[-1 - run_len] == before[-1]:
                    run_len += 1
                inside_advance += run_len < S
    assert inside_advance > 0


# ---- 3: backpointer 127 with the stay bit at unit 0 --------------------------------------------------------------------------
def test_backpointer_127_with_the_stay_bit_at_unit_zero_is_not_a_bad_frame():
    """K = 128, S = 8: unit 0 is entered from unit 127 and then stays, and 127 remains the best unit to enter 0 from, so the
    byte of (frame, unit 0) holds backpointer 127 and the stay bit: 0xFF, which marks a BAD frame in abnz_hmm_dense_viterbi's
    workspace.  Here it must be read as what it is."""
    K, S, D = 128, 8, 1
    lens = (300, 40)
    off, T = layout(lens)
    x = np.zeros((T, D), dtype=np.float32)
    for o, n in zip(off, lens):
        x[o:o + n // 2], x[o + n // 2:o + n] = 1.0, -1.0
    A = np.zeros((K, D), dtype=np.float32)
    A[127], A[0] = 2.0, -2.0                                       # 127 likes x = +1, 0 likes x = -1
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = np.full(K, -16.0, dtype=np.float32)
    c0[[0, 127]] = 0.0
    li = np.full(K, -5.0, dtype=np.float32)
    li[127] = 0.0
    lt = np.full((K, K), -3.0, dtype=np.float32)
    lt[np.arange(K), np.arange(K)] = 0.0
    lt[127, 0] = 0.0
    x64 = x.astype(np.float64)
    s = (x64 @ A.astype(np.float64).T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)).astype(np.float32)
    c = dict(x=x, A=A, B=B, c0=c0, li=li, lt=lt, s=s)
    ids, lp, nsw, ng = check_exact(c, off, lens, S)
    for o, n in zip(off, lens):
        assert ids[o:o + n].tolist() == [127] * (n // 2) + [0] * (n - n // 2)
    assert nsw.tolist() == [1, 1] and ng.tolist() == list(lens)
    r = raw(c, off, lens, S)
    assert same(r, (ids, lp, nsw, ng))


# ---- 4: min_duration = 1 is abnz_hmm_dense_viterbi -----------------------------------------------------------------------------
@pytest.fixture(scope='module')
def float_cases():
    cache = {}

    def get(K):
        if K not in cache:
            rng = np.random.default_rng(K)
            lens = rng.integers(100, 301, size=5)
            x, shift, w, m, v = recipe(K, 40, lens, seed=4000 + K, run_len=7)
            cache[K] = (lens, x, shift, w, Scores(x, shift, w, m, v))
        return cache[K]
    return get


@pytest.mark.parametrize('K', [5, 65, 128])
def test_minimum_duration_one_through_the_new_entry_is_the_twin_bit_for_bit(float_cases, K):
    from abnet3_amd import hmm
    lens, x, shift, w, sc = float_cases(K)
    off = np.cumsum(lens) - lens
    li, lt = hmm.log_transitions(*random_transitions(K, 9 * K, 0.5))
    c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, li=li, lt=lt)
    twin = [host(t) for t in hmm.dense_viterbi(dev(x), off, lens, dev(shift), dev(sc.A), dev(sc.B), dev(sc.c0), dev(li), dev(lt))]
    got = raw(c, off, lens, 1, fill=-1, shift=shift)
    assert same(got, twin) and np.array_equal(got[3], lens)
    assert same(run(c, off, lens, 1, shift=shift), twin)                       # and the Python layer's default route


# ---- 5: random float data against the float64 optimum ----------------------------------------------------------------------
@pytest.mark.parametrize('K,S', [(K, S) for K in (5, 37, 128) for S in (2, 5)])
def test_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K, S):
    from abnet3_amd import hmm
    lens, x, shift, w, sc = float_cases(K)
    off = np.cumsum(lens) - lens
    assert not sc.bad.any()
    used_path, used_lp = 0.0, 0.0
    init, trans = random_transitions(K, 7 * K, 0.5)
    li, lt = hmm.log_transitions(init, trans)
    c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, li=li, lt=lt)
    ids, lp, nsw, ng = run(c, off, lens, S, shift=shift)
    lmax = dd.table_max(li, lt)
    assert np.array_equal(ng, lens)
    for u, (o, n) in enumerate(zip(off, lens)):
        sl = slice(o, o + n)
        good = np.ones(n, dtype=bool)
        opt = dd.optimum_f64(sc.s64[sl], good, li, lt, S)
        allow = 2.0 * n * dd.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax, S)
        j64 = dd.J_runs(sc.s64[sl], ids[sl], good, li, lt, S)
        print('K %d S %d utterance %d: optimum - J_runs(ids) = %.3g, |log_prob - optimum| = %.3g, the bar 2 n_good delta = %.3g'
              % (K, S, u, opt - j64, abs(lp[u] - opt), allow))
        used_path, used_lp = max(used_path, (opt - j64) / allow), max(used_lp, abs(lp[u] - opt) / allow)
        assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (the upper side: float64 rounding of the two sums only)
        assert abs(lp[u] - opt) <= allow
        assert vit_dur_np.run_lengths_ok(ids[sl], S)
        assert nsw[u] == len(dd.runs(ids[sl])) - 1 == dv.switches(ids[sl])
    print('K %d S %d: the largest share of the bar used: path %.3g, log_prob %.3g' % (K, S, used_path, used_lp))


# ---- 6: the sticky matrix against abnx_hmm_viterbi_dur -----------------------------------------------------------------------
@pytest.mark.parametrize('K,S', [(K, S) for K in (5, 37) for S in (2, 4)])
def test_sticky_matrix_gives_the_sticky_twins_log_prob(K, S):
    """lt[j][k] = lr[k] off the diagonal and ls[k] on it, tables in eighths with S ls[k] > lr[k] for every k: the sticky
    decoder's optimum then never closes a unit to enter it again (tests/vit_dur_np.py), so both decoders maximise the same
    score over the same paths, and on exact inputs every value is exact."""
    from abnet3_amd import hmm
    lens = np.array([1, 2, S, S + 1, 127, 128, 129, 300])
    off, T = layout(lens)
    c = exact_case(T, K, 15, seed=600 + K + S)
    rng = np.random.default_rng(K * S)
    ls = (-rng.integers(0, 3, size=K) / 8.0).astype(np.float32)
    lr = (-rng.integers(9, 25, size=K) / 8.0).astype(np.float32)
    assert (S * ls.astype(np.float64) > lr).all() and (ls >= lr).all()
    lw = c['li']
    lt = dv.sticky_log_transitions(ls, lr)
    d = [dev(a) for a in (c['x'], np.zeros(15), c['A'], c['B'], c['c0'])]
    ref = [host(t) for t in hmm.viterbi(d[0], off, lens, d[1], d[2], d[3], d[4], dev(lw), dev(ls), dev(lr), min_duration=S)]
    got = [host(t) for t in hmm.dense_viterbi(d[0], off, lens, d[1], d[2], d[3], d[4], dev(lw), dev(lt), min_duration=S)]
    assert np.array_equal(bits(got[1]), bits(ref[1])) and np.array_equal(got[3], ref[3]) and np.array_equal(got[3], lens)
    for u, (o, n) in enumerate(zip(off, lens)):
        sl = slice(o, o + n)
        good = np.ones(n, dtype=bool)
        assert dd.J_runs(c['s'][sl], got[0][sl], good, lw, lt, S) == got[1][u]
        assert vit_dur_np.J_runs(c['s'][sl], ref[0][sl], good, lw, ls, lr, S) == got[1][u]
        assert dd.J_runs(c['s'][sl], ref[0][sl], good, lw, lt, S) == got[1][u]     # the twin's ids have distinct neighbouring runs by construction
    assert got[2].sum() > 0


# ---- 7: memory and independence ----------------------------------------------------------------------------------------------
def test_more_utterances_than_workgroups_reuse_the_regions():
    n, S = 600, 2
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 6, size=n)
    off = 1 + 6 * np.arange(n, dtype=np.int64)
    T = 6 * n + 1
    c = exact_case(T, 5, 4, seed=4)
    ids, lp, nsw, ng = check_exact(c, off, lens, S)
    inside = inside_rows(T, off, lens)
    assert (ids[~inside] == -7).all() and (~inside).sum() >= n and nsw.max() > 0
    again = run(c, off, lens, S, ids=prefilled(T))
    assert same((ids, lp, nsw, ng), again)
    only = run(c, off, lens, S, ids=prefilled(T), want_log_prob=False)
    assert np.array_equal(only[0], ids) and only[1] is None and only[2] is None and np.array_equal(only[3], ng)


def test_two_calls_are_bit_identical_and_other_rows_are_untouched():
    from abnet3_amd import hmm
    import gmm_np
    import hmm_np
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 400, size=40)
    off, T = layout(lens, gap=3)
    K, D, S = 100, 40, 5
    x, shift, w, m, v = recipe(K, D, [T], seed=8, run_len=6)
    sc_A, sc_B, _ = gmm_np.tables(w, m, v)
    li, lt = hmm.log_transitions(*random_transitions(K, 8, 0.8))
    c = dict(x=x, A=sc_A, B=sc_B, c0=hmm_np.emission_offsets(m, v), li=li, lt=lt)
    sentinel = torch.arange(T, dtype=torch.int32, device='cuda') - 100000
    a = run(c, off, lens, S, ids=sentinel.clone(), shift=shift)
    b = run(c, off, lens, S, ids=sentinel.clone(), shift=shift)
    assert same(a, b)
    inside = inside_rows(T, off, lens)
    assert np.array_equal(a[0][~inside], host(sentinel)[~inside]) and (~inside).sum() >= 3 * 41
    assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()
    assert all(dd.run_lengths_ok(a[0][o:o + n], S) for o, n in zip(off, lens))
    # an utterance alone gives the rows it gave among its neighbours
    u = int(np.argmax(lens))
    one = run(dict(c, x=x[off[u]:off[u] + lens[u]]), [0], [lens[u]], S, shift=shift)
    assert np.array_equal(one[0], a[0][off[u]:off[u] + lens[u]]) and bits(one[1])[0] == bits(a[1])[u] and one[2][0] == a[2][u]


def test_refused_utterances_are_left_untouched_and_their_neighbours_unaffected():
    K, D, T, S = 5, 13, 400, 3
    c = exact_case(T, K, D, seed=17)
    off = np.array([0, -1, 10, T - 3, 30, 340], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300, 50], dtype=np.int32)      # fine, off < 0, len < 0, past the end, longer than the workspace holds, fine
    ids, lp, nsw, ng = raw(c, off, lens, S, ws_len=100)
    assert list(ng) == [5, -1, -1, -1, -1, 50] and list(nsw[1:5]) == [-1] * 4 and np.isnan(lp[1:5]).all()
    assert (ids[5:340] == -7).all() and (ids[390:] == -7).all()
    ref = dd.viterbi(c['s'], np.ones(T, dtype=bool), [0, 340], [5, 50], c['li'], c['lt'], S)
    assert np.array_equal(ids, ref[0]) and np.array_equal(lp[[0, 5]], ref[1]) and np.array_equal(nsw[[0, 5]], ref[2])
    alone = raw(c, [0, 340], [5, 50], S)
    assert np.array_equal(alone[0], ids) and np.array_equal(alone[1], lp[[0, 5]])


# ---- 8: dirty memory -----------------------------------------------------------------------------------------------------------
def test_every_next4_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT4_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT4_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS))


@pytest.mark.parametrize('K', [5, 65])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(K):
    """The entry of DIRTY_CASES with ids, the per-utterance outputs and the workspace from torch.empty under the three
    patterns: the same bits (rows outside every utterance keep the pattern), and they are the restatement's."""
    from abnet3_amd import _lib
    S = 3
    lens = np.array([1, 2, 127, 128, 129, 290], dtype=np.int64)              # a gap of two rows behind every utterance but the last
    off = np.array([0, 3, 7, 136, 266, 397], dtype=np.int64)
    T = int(off[-1] + lens[-1])
    c = exact_case(T, K, 40, seed=K)
    bad = np.zeros(T, dtype=bool)
    bad[[8, 140, 263, 266, 400, 524, 525]] = True                           # BAD frames leave their backpointer rows unwritten
    c['x'][bad] = np.nan
    inside = inside_rows(T, off, lens)
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                r = raw(c, off, lens, S, fill=None)
            assert int(count) >= 5 and count.nbytes > T * 4                  # ids, three outputs and the workspace
            word = int.from_bytes(bytes([byte]) * 4, 'little')
            assert (bits(r[0][~inside]).view(np.uint32) == word).all() and (~inside).sum() == 10
            outs[byte] = [r[0][inside]] + list(r[1:])
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs[byte], outs[0x00])), hex(byte)
    ref = dd.viterbi(c['s'], ~bad, off, lens, c['li'], c['lt'], S)
    assert np.array_equal(outs[0xFF][0], ref[0][inside]) and all(np.array_equal(a, b) for a, b in zip(outs[0xFF][1:], ref[1:]))


# ---- 9: the public layer -----------------------------------------------------------------------------------------------------
def test_decode_and_quantize_with_a_minimum_duration_and_downstream():
    from abnet3_amd import eskmeans, gmm, hmm, kmeans, tde
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    S = 3
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=40, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    w = np.maximum(g.weights_, 1e-8)
    trans = np.full((8, 8), 1.0 / 8)                                            # equal rows: without a minimum duration the frame-wise argmax
    h = hmm.TransitionHmmPosteriorgram(g, trans, w / w.sum())
    free = h.decode(corpus)
    free_lp, free_nsw = h.last_log_prob_.copy(), h.last_n_switch_.copy()
    same_ids = h.decode(corpus, min_duration=1)                                 # the default is today's call
    assert all(np.array_equal(free[k], same_ids[k]) for k in free) and np.array_equal(bits(h.last_log_prob_), bits(free_lp))
    ids = h.decode(corpus, min_duration=S)
    assert list(ids) == corpus.names and h.last_log_prob_.shape == (len(corpus.names),)
    assert h.last_log_prob_.dtype == np.float64 and h.last_n_switch_.dtype == np.int32 and h.last_n_good_.dtype == np.int32
    assert h.n_bad_ == 0 and h.last_n_good_.tolist() == [corpus.length[k] for k in corpus.names]
    for i, k in enumerate(corpus.names):
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],) and (ids[k] >= 0).all() and (ids[k] < 8).all()
        assert dd.run_lengths_ok(ids[k], S) and h.last_n_switch_[i] == len(dd.runs(ids[k])) - 1
    assert not all(dd.run_lengths_ok(free[k], S) for k in free)                 # (without it this corpus does have shorter units)
    nsw = h.last_n_switch_.copy()
    assert nsw.sum() < free_nsw.sum()
    one = corpus.names[0]
    alone = h.decode(dev(feats[one]), min_duration=S)                           # a table: ONE utterance
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.int32 and np.array_equal(host(alone), ids[one])
    # downstream: what the other decoders' ids feed
    seq = kmeans.unit_sequences(ids)
    assert 0.0 < kmeans.bitrate(seq, corpus.total / 100.0) < np.inf
    seg = kmeans.segments(ids)
    assert all(np.array_equal(seg[k][2], seq[k]) and int((seg[k][1] - seg[k][0]).sum()) == corpus.length[k] for k in ids)
    lm = eskmeans.landmarks_from_units(seg, {k: corpus.length[k] for k in corpus.names})
    assert set(lm) == set(corpus.names) and all(lm[k][0] == 0 and lm[k][-1] == corpus.length[k] for k in lm)
    assert set(tde.unit_boundaries(ids, times)) == set(corpus.names)
    counts = hmm.bigram_counts(ids, 8)
    assert counts.shape == (8, 8) and counts.sum() == corpus.total - len(corpus.names)
    assert counts.sum() - np.trace(counts) == nsw.sum()
    quant = h.quantize(corpus, min_duration=S)
    assert isinstance(quant, DeviceCorpus) and quant.names == corpus.names and quant.total == corpus.total
    flat = np.concatenate([ids[k] for k in corpus.names])
    assert np.array_equal(host(quant.table), g.means_.astype(np.float32)[flat])
    # a BAD frame: id -1 and a row of zeros, and the units around it still last
    broken = {k: v.copy() for k, v in feats.items()}
    broken[one][2, 1] = np.nan
    bids = h.decode(broken, min_duration=S)
    assert bids[one][2] == -1 and (np.delete(bids[one], 2) >= 0).all() and h.n_bad_ == 1 and dd.run_lengths_ok(bids[one], S)
    assert not host(h.quantize(DeviceCorpus(broken, times), min_duration=S).table)[corpus.offset[one] + 2].any()
