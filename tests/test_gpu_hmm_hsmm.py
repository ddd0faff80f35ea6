"""abnu_hmm_hsmm_viterbi, abnu_hmm_run_stats and TransitionHmmPosteriorgram's explicit durations on the MI355X against
tests/hmm_hsmm_np.py.

Exact inputs are tests/test_gpu_hmm_dense_vit.py's (`exact_case`: integer frames, tables in eighths) with duration tables in
eighths beside them: every fp32 operation of the score GEMM and of the recurrence is then exact, ties are plentiful, and ids,
log_prob, n_switch and n_good must EQUAL the restatement's.  Random float data is compared through the float64 score with the
allowance hmm_hsmm_np's docstring derives (2 (n_good + 1) delta).  The run statistics are integers and must equal the
restatement's for any grid and any order."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import hmm_hard_np as hh  # noqa: E402
import hmm_hsmm_np as hs  # noqa: E402
from test_gpu_hmm_vit import dev, host, layout, mixture, prefilled, recipe, Scores  # noqa: E402
from test_gpu_hmm_dense_vit import exact_case, inside_rows, random_transitions  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT6_SYMBOLS: the entries the dirty-memory tests below reach, and the host queries
DIRTY_CASES = ('abnu_hmm_hsmm_viterbi', 'abnu_hmm_run_stats')
QUERIES = ('abnu_hmm_hsmm_max_duration', 'abnu_hmm_hsmm_viterbi_ws_bytes')

KS = (1, 2, 3, 16, 17, 64, 65, 128)                           # every capacity (16, 32, 64, 128), at both edges
LS = (2, 7, 8, 9, 16, 17, 31, 32)                             # every register capacity of the chain (8, 16, 32), at both edges
DS = (1, 40, 127)
bits = dirty_memory.bits


def lengths_for(L):
    return (1, 2, L, L + 1, 127, 128, 129, 300)


def with_durations(c, L, seed):
    """exact_case's dict with lx (its lt: the diagonal is never read), ld [K, L] and ls [K] in eighths."""
    rng = np.random.default_rng(seed)
    K = len(c['c0'])
    c = dict(c, lx=c['lt'])
    c['ld'] = (-rng.integers(0, 25, size=(K, L)) / 8.0).astype(np.float32)
    c['ls'] = (-rng.integers(0, 9, size=K) / 8.0).astype(np.float32)
    return c


def run(c, off, lens, ids=None, shift=None, want_log_prob=True):
    from abnet3_amd import hmm
    D = c['x'].shape[1]
    shift = np.zeros(D, dtype=np.float32) if shift is None else shift
    out = hmm.hsmm_viterbi(dev(c['x']), off, lens, dev(shift), dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['li']), dev(c['lx']),
                           dev(c['ld']), dev(c['ls']), ids=ids, want_log_prob=want_log_prob)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


def raw(c, off, lens, ws_len=None, fill=-7, shift=None):
    """(ids, log_prob, n_switch, n_good) host arrays of abnu_hmm_hsmm_viterbi with the per-utterance outputs and the workspace
    from torch.empty, ids from torch.empty filled with `fill` (None: left as torch.empty gave it)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    T, D = c['x'].shape
    K, n, L = len(c['c0']), len(off), c['ld'].shape[1]
    d = {k: dev(c[k]) for k in ('x', 'A', 'B', 'c0', 'li', 'lx', 'ld', 'ls')}
    shift = dev(np.zeros(D) if shift is None else shift)
    ids = torch.empty(T, dtype=torch.int32, device='cuda')
    if fill is not None:
        ids.fill_(fill)
    lp = torch.empty(n, dtype=torch.float64, device='cuda')
    nsw = torch.empty(n, dtype=torch.int32, device='cuda')
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    need = lib.abnu_hmm_hsmm_viterbi_ws_bytes(n, max(1, int(np.max(lens))) if ws_len is None else ws_len, K, D, L)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    rc = lib.abnu_hmm_hsmm_viterbi(p(d['x']), T, D, p(off_d), p(len_d), n, p(shift), p(d['A']), p(d['B']), p(d['c0']), p(d['li']),
                                   p(d['lx']), K, p(ids), p(lp), p(nsw), p(ng), p(ws), need, _lib.stream(), p(d['ld']), p(d['ls']), L)
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(ids), host(lp), host(nsw), host(ng)


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


def check_exact(c, off, lens, good=None):
    T = c['x'].shape[0]
    good = np.ones(T, dtype=bool) if good is None else good
    ref = hs.viterbi(c['s'], good, off, lens, c['li'], c['lx'], c['ld'], c['ls'])
    got = run(c, off, lens, ids=prefilled(T))
    assert np.array_equal(got[0], ref[0]), np.flatnonzero(got[0] != ref[0])[:10]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].dtype == np.int32
    return got


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,L,D', [(K, L, D) for K in KS for L in LS for D in DS])
def test_exact_inputs_equal_the_restatement(K, L, D):
    lens = np.array(lengths_for(L))[::-1]                       # laid out with gaps ...
    off, T = layout(lens)
    c = with_durations(exact_case(T, K, D, seed=1000 * K + 10 * D + L), L, seed=K + L)
    order = np.argsort(-off)                                     # ... and handed over with descending offsets
    ids, lp, nsw, ng = check_exact(c, off[order], lens[order])
    assert np.array_equal(ng, lens[order])
    inside = inside_rows(T, off, lens)
    assert (ids[~inside] == -7).all() and (ids[inside] >= 0).all() and (ids[inside] < K).all()
    assert all(nsw[u] == len(hs.runs(ids[o:o + n])) - 1 for u, (o, n) in enumerate(zip(off[order], lens[order])))
    assert K < 3 or D == 1 or nsw.sum() > 0                      # (one feature or two units: a single unit may win throughout)
    # the same utterances handed over in another order: the same rows get the same ids
    perm = np.random.default_rng(K + D + L).permutation(len(lens))
    ids2, lp2, nsw2, ng2 = run(c, off[perm], lens[perm], ids=prefilled(T))
    back = np.argsort(order)[perm]
    assert np.array_equal(ids2, ids) and np.array_equal(lp2, lp[back]) and np.array_equal(nsw2, nsw[back]) and np.array_equal(ng2, ng[back])


# ---- 2: BAD frames ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,L', [(5, 2), (5, 9), (65, 8), (128, 32)])
def test_bad_frames_with_exact_inputs_equal_the_restatement(K, L):
    lens = (140, 5, 300, 3, 300, 90)
    off, T = layout(lens)
    c = with_durations(exact_case(T, K, 15, seed=33 + K + L), L, seed=7 * K + L)
    bad = np.zeros(T, dtype=bool)
    # first / middle / last; none; rows 127 and 128; all; a run across the first block edge, one up to the second and the last
    # row; single BAD frames every few rows (inside segments' heads) and a run longer than L
    for u, rows in enumerate(([0, 70, 139], [], [127, 128, 200], [0, 1, 2], list(range(120, 135)) + list(range(250, 256)) + [299],
                              list(range(3, 40, 4)) + list(range(50, 50 + min(L, 8) + 3)))):
        bad[off[u] + np.array(rows, dtype=np.int64)] = True
    c['x'][bad] = np.nan
    c['x'][off[2] + 128, 1:] = 0.0                                                    # one NaN entry is enough
    c['x'][off[0]] = np.inf
    got = check_exact(c, off, lens, ~bad)
    inside = inside_rows(T, off, lens)
    assert np.array_equal(got[0] == -1, bad) and (got[0][inside & ~bad] >= 0).all()
    assert got[1][3] == 0.0 and got[2][3] == 0 and got[3][3] == 0
    assert got[3].tolist() == [137, 5, 297, 0, 300 - 22, 90 - 10 - (min(L, 8) + 3)]
    # a BAD frame did fall inside a segment: the same unit on both sides of it
    ref = got[0]
    inside_segment = 0
    for o, n in zip(off, lens):
        row = ref[o:o + n]
        for r in np.flatnonzero(row == -1):
            before, after = row[:r][row[:r] >= 0], row[r + 1:][row[r + 1:] >= 0]
            inside_segment += bool(len(before) and len(after) and before[-1] == after[0])
    assert inside_segment > 0 or K > 5                          # (many units: the segments are short, and none may hold a BAD frame)


# ---- 3: constructed cases ----------------------------------------------------------------------------------------------------
def flat_case(T, K, D, L):
    """Every score and every table entry 0: every compare of the recurrence is a tie."""
    z = lambda *shape: np.zeros(shape, dtype=np.float32)
    return dict(x=z(T, D), A=z(K, D), B=z(K, D), c0=z(K), li=z(K), lx=z(K, K), ld=z(K, L), ls=z(K), s=z(T, K))


@pytest.mark.parametrize('K,L', [(1, 2), (2, 2), (5, 4), (17, 9), (128, 32)])
def test_ties_everywhere_go_the_restatements_way(K, L):
    """All zero: xi ties over every state (the lowest wins), bp over every unit (the lowest other unit wins), the tail's stay
    against the advance (the advance wins), N_t and the final state over every unit."""
    lens = np.array([1, 2, L, L + 1, 2 * L + 3, 130, 257])
    off, T = layout(lens)
    c = flat_case(T, K, 3, L)
    ids, lp, nsw, ng = check_exact(c, off, lens)
    assert (lp == 0.0).all() and np.array_equal(ng, lens)
    # the same ties at constant, non-zero tables: staying in the tail is free, every switch and every closed segment costs
    c['ld'][:] = -0.5
    c['lx'][:] = -0.5
    ids, lp, nsw, ng = check_exact(c, off, lens)
    assert (nsw == 0).all() and (lp == -0.5).all()


def test_the_optimum_sits_in_the_tail_for_more_than_128_frames():
    K, L, D = 3, 4, 1
    lens = (300, 129, 131)
    off, T = layout(lens)
    x = np.ones((T, D), dtype=np.float32)
    A = np.zeros((K, D), dtype=np.float32)
    B = np.zeros((K, D), dtype=np.float32)
    c0 = np.array([0.0, -16.0, -16.0], dtype=np.float32)
    li = np.zeros(K, dtype=np.float32)
    lx = np.full((K, K), -1.0, dtype=np.float32)
    ld = np.full((K, L), -0.5, dtype=np.float32)
    ls = np.array([-0.125, -0.25, -0.25], dtype=np.float32)
    s = np.tile(c0, (T, 1))
    c = dict(x=x, A=A, B=B, c0=c0, li=li, lx=lx, ld=ld, ls=ls, s=s)
    ids, lp, nsw, ng = check_exact(c, off, lens)
    for u, (o, n) in enumerate(zip(off, lens)):
        assert (ids[o:o + n] == 0).all() and nsw[u] == 0
        assert lp[u] == -0.5 + (n - L) * -0.125                                      # one segment: log p_0(n), exactly
    # the same with a BAD frame on each side of the block edge inside the tail
    bad = np.zeros(T, dtype=bool)
    bad[off[0] + np.array([127, 128, 255, 256])] = True
    c['x'][bad] = np.nan
    ids, lp, nsw, ng = check_exact(c, off, lens, ~bad)
    assert lp[0] == -0.5 + (296 - L) * -0.125 and ng[0] == 296 and nsw[0] == 0


@pytest.mark.parametrize('L', [2, 8, 32])
def test_backpointer_127_with_the_last_duration_state(L):
    """K = 128: unit 127 holds the first half of the utterance -- longer than L, so it is left from its tail state, xi = L --
    and unit 0 the second, so the byte of (the switch frame, unit 0) holds backpointer 127, later with the stay bit (0xFF), and
    the xi byte of (the switch frame, unit 127) holds L."""
    K, D = 128, 1
    lens = (300, 2 * L + 8)
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
    lx = np.full((K, K), -3.0, dtype=np.float32)
    lx[127, 0] = 0.0
    ld = np.zeros((K, L), dtype=np.float32)
    ls = np.zeros(K, dtype=np.float32)
    x64 = x.astype(np.float64)
    s = (x64 @ A.astype(np.float64).T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)).astype(np.float32)
    c = dict(x=x, A=A, B=B, c0=c0, li=li, lx=lx, ld=ld, ls=ls, s=s)
    ids, lp, nsw, ng = check_exact(c, off, lens)
    for o, n in zip(off, lens):
        assert ids[o:o + n].tolist() == [127] * (n // 2) + [0] * (n - n // 2)
    assert nsw.tolist() == [1, 1] and ng.tolist() == list(lens)
    # the restatement's own record at the switch frame: entered from 127 in its state L
    o, n = int(off[1]), int(lens[1])
    V = None
    for t in range(n // 2):                                        # unit 127's chain over the first half, by the module's formulas
        U = np.full((K, L), -np.inf, dtype=np.float32)
        if V is None:
            U[:, 0] = s[o + t] + li
        else:
            xx, _ = hs.exit_max(V, ld)
            cand = xx[:, None] + np.where(np.eye(K, dtype=bool), -np.inf, lx).astype(np.float32)
            a, below = V[:, L - 1] + ls, V[:, L - 2]
            U[:, L - 1] = s[o + t] + np.where(a > below, a, below)
            for i in range(L - 2, 0, -1):
                U[:, i] = s[o + t] + V[:, i - 1]
            U[:, 0] = s[o + t] + cand.max(axis=0)
        V = U - U.max()
    xx, xi = hs.exit_max(V, ld)
    cand = xx + lx[:, 0]
    cand[0] = -np.inf
    assert int(np.argmax(cand)) == 127 and int(xi[127]) == L - 1
    r = raw(c, off, lens)
    assert same(r, (ids, lp, nsw, ng))


# ---- 4: random float data against the float64 optimum ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def float_cases():
    cache = {}

    def get(K):
        if K not in cache:
            rng = np.random.default_rng(K)
            lens = rng.integers(100, 301, size=5)
            x, shift, w, m, v = recipe(K, 40, lens, seed=6000 + K, run_len=7)
            cache[K] = (lens, x, shift, w, Scores(x, shift, w, m, v))
        return cache[K]
    return get


def random_durations(K, L, seed):
    rng = np.random.default_rng(seed)
    return rng.dirichlet(np.full(L, 1.0), size=K) * (1.0 - 1e-6) + 1e-6 / L, rng.uniform(0.2, 0.95, size=K)


@pytest.mark.parametrize('K,L', [(5, 3), (37, 8), (65, 17), (128, 32)])
def test_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K, L):
    from abnet3_amd import hmm
    lens, x, shift, w, sc = float_cases(K)
    off = np.cumsum(lens) - lens
    assert not sc.bad.any()
    used_path, used_lp = 0.0, 0.0
    li, lx = hmm.switch_log_transitions(*random_transitions(K, 7 * K, 0.5))
    ld, ls = hmm.duration_tables(*random_durations(K, L, K + L))
    c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, li=li, lx=lx, ld=ld, ls=ls)
    ids, lp, nsw, ng = run(c, off, lens, shift=shift)
    lmax = hs.table_max(li, lx, ld, ls)
    assert np.array_equal(ng, lens)
    for u, (o, n) in enumerate(zip(off, lens)):
        sl = slice(o, o + n)
        good = np.ones(n, dtype=bool)
        opt = hs.viterbi_one(sc.s64[sl], good, li, lx, ld, ls, np.float64)[1]
        allow = 2.0 * (n + 1) * hs.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax, L)
        j64 = hs.J_runs(sc.s64[sl], ids[sl], good, li, lx, ld, ls)
        print('K %d L %d utterance %d: optimum - J_runs(ids) = %.3g, |log_prob - optimum| = %.3g, the bar 2 (n_good + 1) delta = %.3g'
              % (K, L, u, opt - j64, abs(lp[u] - opt), allow))
        used_path, used_lp = max(used_path, (opt - j64) / allow), max(used_lp, abs(lp[u] - opt) / allow)
        assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (the upper side: float64 rounding of the two sums only)
        assert abs(lp[u] - opt) <= allow
        assert nsw[u] == len(hs.runs(ids[sl])) - 1
    print('K %d L %d: the largest share of the bar used: path %.3g, log_prob %.3g' % (K, L, used_path, used_lp))


# ---- 5: memory and independence ----------------------------------------------------------------------------------------------
def test_two_grids_give_the_same_bits_and_the_regions_are_reused():
    n, L = 600, 3
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 6, size=n)
    off = 1 + 6 * np.arange(n, dtype=np.int64)
    T = 6 * n + 1
    c = with_durations(exact_case(T, 5, 4, seed=4), L, seed=4)
    ids, lp, nsw, ng = check_exact(c, off, lens)                       # 256 workgroups, each two or three utterances
    inside = inside_rows(T, off, lens)
    assert (ids[~inside] == -7).all() and (~inside).sum() >= n and nsw.max() > 0
    part = prefilled(T)
    pieces = [run(c, off[i:i + 100], lens[i:i + 100], ids=part) for i in range(0, n, 100)]       # 100 workgroups, six times
    assert np.array_equal(pieces[-1][0], ids)
    assert same([np.concatenate([p[k] for p in pieces]) for k in (1, 2, 3)], (lp, nsw, ng))
    only = run(c, off, lens, ids=prefilled(T), want_log_prob=False)
    assert np.array_equal(only[0], ids) and only[1] is None and only[2] is None and np.array_equal(only[3], ng)


def test_two_calls_are_bit_identical_and_an_utterance_alone_gives_its_rows():
    from abnet3_amd import hmm
    import gmm_np
    import hmm_np
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 400, size=40)
    off, T = layout(lens, gap=3)
    K, D, L = 100, 40, 12
    x, shift, w, m, v = recipe(K, D, [T], seed=8, run_len=6)
    sc_A, sc_B, _ = gmm_np.tables(w, m, v)
    li, lx = hmm.switch_log_transitions(*random_transitions(K, 8, 0.8))
    ld, ls = hmm.duration_tables(*random_durations(K, L, 5))
    c = dict(x=x, A=sc_A, B=sc_B, c0=hmm_np.emission_offsets(m, v), li=li, lx=lx, ld=ld, ls=ls)
    sentinel = torch.arange(T, dtype=torch.int32, device='cuda') - 100000
    a = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    b = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    assert same(a, b)
    inside = inside_rows(T, off, lens)
    assert np.array_equal(a[0][~inside], host(sentinel)[~inside]) and (~inside).sum() >= 3 * 41
    assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()
    for u in (int(np.argmax(lens)), int(np.argmin(lens)), 7):         # alone: a grid of one, no neighbours
        one = run(dict(c, x=x[off[u]:off[u] + lens[u]]), [0], [lens[u]], shift=shift)
        assert np.array_equal(one[0], a[0][off[u]:off[u] + lens[u]]) and bits(one[1])[0] == bits(a[1])[u] and one[2][0] == a[2][u]


def test_refused_utterances_are_left_untouched_and_their_neighbours_unaffected():
    K, D, T, L = 5, 13, 400, 3
    c = with_durations(exact_case(T, K, D, seed=17), L, seed=17)
    off = np.array([0, -1, 10, T - 3, 30, 340], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300, 50], dtype=np.int32)      # fine, off < 0, len < 0, past the end, longer than the workspace holds, fine
    ids, lp, nsw, ng = raw(c, off, lens, ws_len=100)
    assert list(ng) == [5, -1, -1, -1, -1, 50] and list(nsw[1:5]) == [-1] * 4 and np.isnan(lp[1:5]).all()
    assert (ids[5:340] == -7).all() and (ids[390:] == -7).all()
    ref = hs.viterbi(c['s'], np.ones(T, dtype=bool), [0, 340], [5, 50], c['li'], c['lx'], c['ld'], c['ls'])
    assert np.array_equal(ids, ref[0]) and np.array_equal(lp[[0, 5]], ref[1]) and np.array_equal(nsw[[0, 5]], ref[2])


# ---- 6: dirty memory -----------------------------------------------------------------------------------------------------------
def test_every_next6_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT6_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT6_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS) |
                                          set(_lib.NEXT4_SYMBOLS) | set(_lib.NEXT5_SYMBOLS))


@pytest.mark.parametrize('K,L', [(5, 3), (65, 20)])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(K, L):
    """Both entries of DIRTY_CASES with every output and the workspace from torch.empty under the three patterns: the same bits
    (rows outside every utterance keep the pattern), and they are the restatement's."""
    from abnet3_amd import _lib
    lens = np.array([1, 2, 127, 128, 129, 290], dtype=np.int64)              # a gap of two rows behind every utterance but the last
    off = np.array([0, 3, 7, 136, 266, 397], dtype=np.int64)
    T = int(off[-1] + lens[-1])
    c = with_durations(exact_case(T, K, 40, seed=K), L, seed=K)
    bad = np.zeros(T, dtype=bool)
    bad[[8, 140, 263, 266, 400, 524, 525]] = True                           # BAD frames leave their byte rows unwritten
    c['x'][bad] = np.nan
    inside = inside_rows(T, off, lens)
    outs, stats = {}, {}
    lib = _lib.load()
    with dirty_memory.recorded(lib) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                r = raw(c, off, lens, fill=None)
            assert int(count) >= 5 and count.nbytes > T * 4                  # ids, three outputs and the workspace
            word = int.from_bytes(bytes([byte]) * 4, 'little')
            assert (bits(r[0][~inside]).view(np.uint32) == word).all() and (~inside).sum() == 10
            outs[byte] = [r[0][inside]] + list(r[1:])
            with dirty_memory.dirty(byte) as count:
                dur = torch.empty((K, L), dtype=torch.int64, device='cuda')
                tail = torch.empty(K, dtype=torch.int64, device='cuda')
            assert int(count) == 2
            ids_d, off_d, len_d = dev(r[0], np.int32), dev(off, np.int64), dev(lens, np.int32)      # (held until the launch is done)
            rc = lib.abnu_hmm_run_stats(_lib.ptr(ids_d), T, _lib.ptr(off_d), _lib.ptr(len_d), len(off), K, L, _lib.ptr(dur), _lib.ptr(tail),
                                        _lib.stream())
            assert rc == 0, lib.abn_last_error()
            torch.cuda.synchronize()
            stats[byte] = (host(dur), host(tail))
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs[byte], outs[0x00])), hex(byte)
        assert np.array_equal(stats[byte][0], stats[0x00][0]) and np.array_equal(stats[byte][1], stats[0x00][1])
    ref = hs.viterbi(c['s'], ~bad, off, lens, c['li'], c['lx'], c['ld'], c['ls'])
    assert np.array_equal(outs[0xFF][0], ref[0][inside]) and all(np.array_equal(a, b) for a, b in zip(outs[0xFF][1:], ref[1:]))
    want = hs.run_stats(ref[0], off, lens, K, L)                             # (rows outside hold the pattern: they count nothing)
    assert np.array_equal(stats[0xFF][0], want[0]) and np.array_equal(stats[0xFF][1], want[1])


# ---- 7: the run statistics -----------------------------------------------------------------------------------------------------
def device_run_stats(ids, off, lens, K, L):
    from abnet3_amd import hmm
    dur, tail = hmm.run_stats(dev(ids, np.int32), off, lens, K, L)
    torch.cuda.synchronize()
    assert dur.dtype == torch.int64 and tail.dtype == torch.int64 and dur.shape == (K, L) and tail.shape == (K,)
    return host(dur), host(tail)


def runny_ids(rng, T, K, mean_run, bad_share):
    """Random ids in runs of geometric length, a share of them BAD (-1, or an id >= K)."""
    ids = np.repeat(rng.integers(0, K, size=T), rng.geometric(1.0 / mean_run, size=T))[:T].astype(np.int32)
    bad = rng.random(T) < bad_share
    ids[bad] = np.where(rng.random(int(bad.sum())) < 0.5, -1, K + rng.integers(0, 3, size=int(bad.sum())))
    return ids


@pytest.mark.parametrize('K,L,mean_run', [(1, 2, 5), (2, 32, 40), (3, 5, 5), (17, 8, 9), (64, 31, 70), (128, 2, 3), (128, 32, 30)])
def test_run_stats_equal_the_restatement_on_random_ids(K, L, mean_run):
    rng = np.random.default_rng(K + L)
    lens = np.concatenate([[0, 1, 2, 63, 64, 65, 127, 128, 129, 1000], rng.integers(1, 200, size=30)])
    off, T = layout(lens, gap=1)
    ids = runny_ids(rng, T, K, mean_run, 0.1)
    want = hs.run_stats(ids, off, lens, K, L)
    got = device_run_stats(ids, off, lens, K, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    assert want[1].sum() > 0 or mean_run < L                              # runs longer than L did occur
    crossing = sum(1 for o, n in zip(off, lens) for e in range(int(o) + 64, int(o) + int(n), 64) if ids[e] == ids[e - 1] and 0 <= ids[e] < K)
    assert crossing > 0                                                      # and runs across the 64-id edges
    perm = rng.permutation(len(lens))                                        # another order of the utterances: the same counts
    again = device_run_stats(ids, off[perm], lens[perm], K, L)
    assert np.array_equal(again[0], want[0]) and np.array_equal(again[1], want[1])


def test_run_stats_with_more_utterances_than_the_grid_holds_and_one_long_run():
    K, L = 7, 6
    rng = np.random.default_rng(1)
    n = 3000                                                                 # 256 workgroups of four waves: three rounds
    lens = rng.integers(0, 12, size=n)
    off, T = layout(lens, gap=1)
    ids = runny_ids(rng, T, K, 4, 0.1)
    want = hs.run_stats(ids, off, lens, K, L)
    got = device_run_stats(ids, off, lens, K, L)
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])
    half = [device_run_stats(ids, off[i::2], lens[i::2], K, L) for i in (0, 1)]          # two smaller grids add up to it
    assert np.array_equal(half[0][0] + half[1][0], want[0]) and np.array_equal(half[0][1] + half[1][1], want[1])
    # one run over many chunks, BAD frames at the chunk edges and inside
    ids = np.full(1000, 3, dtype=np.int32)
    ids[[0, 63, 64, 65, 127, 128, 500, 999]] = -1
    dur, tail = device_run_stats(ids, [0], [1000], K, L)
    assert dur.sum() == 1 and dur[3, L - 1] == 1 and tail.tolist() == [0, 0, 0, 992 - L, 0, 0, 0]


# ---- 8: the training loop --------------------------------------------------------------------------------------------------------
def planted_model(alpha=0.0):
    from abnet3_amd import hmm
    x, lens, means, z = hs.planted_corpus()
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    m0, v0, t0, i0 = hh.planted_start(means, 0)
    g = mixture(shift, np.full(4, 0.25), m0 - shift.astype(np.float64), v0)
    g.gv_ = x.astype(np.float64).var(axis=0)
    names = ['u%02d' % i for i in range(len(lens))]
    off = np.cumsum(lens) - lens
    feats = {k: x[o:o + n] for k, o, n in zip(names, off, lens)}
    return hmm.TransitionHmmPosteriorgram(g, t0, i0, alpha=alpha), feats, names, x, lens, off, shift, z


def slack_of(h, x, shift):
    """The decoder's per-frame slack under h's parameters: delta of tests/hmm_hsmm_np.py."""
    from abnet3_amd import hmm
    g = h.gmm
    sc = Scores(x, shift, np.full(4, 0.25), g.means_ - shift.astype(np.float64), g.variances_)
    li, lx = hmm.switch_log_transitions(h.init_, h.trans_)
    ld, ls = hmm.duration_tables(h.dur_, h.dur_tail_)
    return hs.delta(sc.E.max(), np.abs(sc.s64).max() + sc.E.max(), hs.table_max(li, lx, ld, ls), h.dur_.shape[1])


def test_fit_viterbi_with_durations_on_the_planted_corpus():
    from abnet3_amd import hmm
    L = hs.PLANTED_L
    h, feats, names, x, lens, off, shift, z = planted_model()
    whole = copy.deepcopy(h).fit_viterbi(feats, n_iter=10, tol=-np.inf, params='mvtid', max_duration=L)
    h.set_durations(max_duration=L)                                            # the geometric start the loop takes
    lps, slacks = [], [slack_of(h, x, shift)]
    table, shift_d = dev(x), dev(shift)
    for it in range(len(whole.viterbi_log_probs)):
        # the iteration by hand: the device's own ids under the current parameters, their statistics, the three host updates
        dec = h.decode(feats, durations=True)
        ids = np.concatenate([dec[k] for k in names])
        lps.append(float(h.last_log_prob_.sum()) / int(h.last_n_good_.sum()))
        counts, sums, ng = (host(t) for t in hmm.hard_stats(table, off, lens, shift_d, dev(ids, np.int32), 4, min_duration=1))
        dur, tail = device_run_stats(ids, off, lens, 4, L)
        ref = hh.hard_stats(x, off, lens, shift, ids, 4, 1, with_abs=True)
        want = hs.run_stats(ids, off, lens, 4, L)
        assert np.array_equal(counts, ref[0]) and np.array_equal(ng, ref[2]) and (np.abs(sums - ref[1]) <= hh.sums_bar(ref[3])).all()
        assert np.array_equal(dur, want[0]) and np.array_equal(tail, want[1])
        assert dur.sum() == h.last_n_switch_.sum() + len(names)                # the runs are the segments
        g = h.gmm
        _, m, v, _, _ = hmm.baum_welch_update(sums, np.zeros(4), 0, g.means_ - shift.astype(np.float64), g.variances_, g.gv_, g.var_floor,
                                              g.min_count, 'mv', weights=np.full(4, 0.25), stay=0.0)
        t, i = hmm.transition_update(counts.astype(np.float64), h.trans_, h.init_, h.alpha, 'ti')
        q, r = hs.duration_update(dur, tail, h.dur_, h.dur_tail_, h.alpha)
        h.fit_viterbi(feats, n_iter=1, params='mvtid')                          # the same iteration through the loop
        assert len(h.viterbi_log_probs) == 1 and abs(h.viterbi_log_probs[0] - lps[-1]) <= 1e-12 * abs(lps[-1])      # (two float64 sums of 12)
        lps[-1] = h.viterbi_log_probs[0]
        assert np.array_equal(h.trans_, t) and np.array_equal(h.init_, i)
        assert np.array_equal(h.gmm.means_, m + shift.astype(np.float64)) and np.array_equal(h.gmm.variances_, v)
        assert np.allclose(h.dur_, q, rtol=1e-14, atol=0) and np.allclose(h.dur_tail_, r, rtol=1e-14, atol=0)
        slacks.append(slack_of(h, x, shift))
    assert np.array_equal(bits(np.array(whole.viterbi_log_probs)), bits(np.array(lps)))       # ten iterations in one call are these
    assert np.array_equal(whole.dur_, h.dur_) and np.array_equal(whole.dur_tail_, h.dur_tail_)
    steps = np.diff(lps)
    n_frames, n_utt = int(sum(lens)), len(lens)
    allow = np.array([(slacks[i] + slacks[i + 1]) * (n_frames + n_utt) / n_frames for i in range(len(steps))])   # 2 (n_good + 1) delta per utterance
    print('viterbi_log_probs %s\n  steps %s\n  slack %s\n  modes %s, tail stay %s'
          % (lps, steps.tolist(), allow.tolist(), (np.argmax(whole.dur_, axis=1) + 1).tolist(), whole.dur_tail_.tolist()))
    # non-decreasing within the decoder's slack (alpha = 0: every M-step is the maximiser of its part of the path score)
    assert len(lps) >= 3 and (steps >= -allow).all() and lps[-1] > lps[0] + 0.1
    want = [min(n, L) for n in hs.PLANTED_LENGTHS]
    assert (np.argmax(whole.dur_, axis=1) + 1).tolist() == want                 # the modes the float64 loop finds on the CPU
    long_unit = int(np.argmax(hs.PLANTED_LENGTHS))
    assert abs(whole.dur_tail_[long_unit] - (hs.PLANTED_LENGTHS[long_unit] - L) / (hs.PLANTED_LENGTHS[long_unit] - L + 1.0)) < 0.02
    final = whole.decode(feats, durations=True)
    assert (np.concatenate([final[k] for k in names]) == z).mean() > 0.99


# ---- 9: the public layer -----------------------------------------------------------------------------------------------------
def test_planted_durations_give_fewer_segments_on_a_noisy_corpus(tmp_path):
    from abnet3_amd import hmm
    from abnet3_amd.dataloader import DeviceCorpus
    rng = np.random.RandomState(3)
    K, L = 4, 8
    means = np.array([[0.0, 0.0], [2.0, 0.0], [2.0, 2.0], [0.0, 2.0]])          # close units: frame-wise decisions flicker
    feats, times = {}, {}
    for u in range(10):
        z = np.repeat((rng.randint(K) + np.cumsum(1 + rng.randint(3, size=9))) % K, 12)
        feats['u%02d' % u] = (means[z] + rng.randn(len(z), 2)).astype(np.float32)
        times['u%02d' % u] = 0.01 * np.arange(len(z))
    x = np.concatenate(list(feats.values()))
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    g = mixture(shift, np.full(K, 0.25), means - shift.astype(np.float64), np.ones((K, 2)))
    h = hmm.TransitionHmmPosteriorgram(g, np.full((K, K), 0.25), np.full(K, 0.25))
    free = h.decode(feats)
    free_nsw = int(h.last_n_switch_.sum())
    q = np.full((K, L), 1e-4)
    q[:, L - 1] = 1.0                                                            # the planted law: 12 frames, in the tail of L = 8
    h.set_durations(q / q.sum(axis=1, keepdims=True), np.full(K, 4.0 / 5.0))
    ids = h.decode(feats, durations=True)
    assert list(ids) == list(feats) and h.last_log_prob_.shape == (10,) and h.last_n_good_.tolist() == [108] * 10
    assert all(ids[k].dtype == np.int32 and ids[k].shape == (108,) and (ids[k] >= 0).all() and (ids[k] < K).all() for k in ids)
    assert all(h.last_n_switch_[i] == len(hs.runs(ids[k])) - 1 for i, k in enumerate(ids))
    assert int(h.last_n_switch_.sum()) < free_nsw                               # fewer segments: the direction only
    again = h.decode(feats)                                                      # the plain path is untouched by the durations
    assert all(np.array_equal(free[k], again[k]) for k in free)
    corpus = DeviceCorpus(feats, times)
    quant = h.quantize(corpus, durations=True)
    flat = np.concatenate([ids[k] for k in corpus.names])
    assert np.array_equal(host(quant.table), g.means_.astype(np.float32)[flat])
    one = list(feats)[0]
    alone = h.decode(dev(feats[one]), durations=True)                            # a table: ONE utterance
    assert isinstance(alone, torch.Tensor) and np.array_equal(host(alone), ids[one])
    # files and the command line
    path, inp, out = str(tmp_path / 'm.npz'), str(tmp_path / 'f.npz'), str(tmp_path / 'ids.npz')
    h.save(path)
    np.savez(inp, **feats)
    assert hmm.main(['decode', path, inp, out, '--durations']) == 0
    with np.load(out) as f:
        assert all(np.array_equal(np.asarray(f[k]).ravel(), ids[k]) for k in ids)
    trained = str(tmp_path / 't.npz')
    assert hmm.main(['fit-trans', path, inp, trained, '--viterbi', '--max-duration', '6', '--params', 'mvtid', '--n-iter', '2']) == 0
    t = hmm.TransitionHmmPosteriorgram.load(trained)
    assert t.dur_.shape == (K, 6) and len(t.viterbi_log_probs) == 2
