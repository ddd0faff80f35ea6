"""abnx_kmeans_viterbi_dur and abnx_hmm_viterbi_dur (the minimum unit duration of the two max-product decoders) on the
MI355X against tests/vit_dur_np.py, and min_duration through the public layer.

Exact inputs (tests/test_gpu_hmm_vit.py's exact_case, tests/units_np.py's exact_case: every fp32 operation of the score
GEMM and of the recurrence exact, ties plentiful): ids, log_prob / objective, n_switch and n_good must EQUAL the
restatement's.  Float data is compared through the float64 optimum with the allowance vit_dur_np's docstring derives
(2 n_good delta).  Every entry is called straight at the library with outputs and workspace from torch.empty, so the same
callers serve the dirty-memory cases; DIRTY_CASES / QUERIES below are the ledger of include/abnet3_hip_next.h."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import gmm_np  # noqa: E402
import hmm_np  # noqa: E402
import hmm_vit_np  # noqa: E402
import kmeans_np  # noqa: E402
import units_np  # noqa: E402
import vit_dur_np  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT_SYMBOLS: the entries the dirty-memory test below reaches, and the one host query
DIRTY_CASES = ('abnx_kmeans_viterbi_dur', 'abnx_hmm_viterbi_dur')
QUERIES = ('abnx_viterbi_dur_max',)

KS, DS, SS = (1, 5, 64, 128, 129, 300), (3, 40), (2, 3, 8)
PLANTED = (62, 127)            # unit boundaries planted in a 300-frame utterance: see plant()


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def layout(lengths, gap=2):
    off, o = [], gap
    for n in lengths:
        off.append(o)
        o += n + gap
    return np.array(off, dtype=np.int64), o


def lengths_for(S):
    """Lengths around every edge (0, 1, the minimum, the 64-frame round, the 128-frame block) in one corpus, and a 300-frame
    utterance for the planted boundaries at its end."""
    return (0, 1, S - 1, S, S + 1, 63, 64, 65, 127, 128, 129, 300, 300)


# ---- the two entries, straight at the library -------------------------------------------------------------------------------
def _outputs(T, n, fill):
    ids = torch.empty(T, dtype=torch.int32, device='cuda')
    if fill is not None:
        ids.fill_(fill)
    return ids, torch.empty(n, dtype=torch.float64, device='cuda'), torch.empty(n, dtype=torch.int32, device='cuda')


def raw_hmm(c, off, lens, S, shift=None, new=True, fill=-7):
    """(ids, log_prob, n_switch, n_good) host arrays of abnx_hmm_viterbi_dur (new=False: abn_hmm_viterbi, S ignored)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    x = dev(c['x'])
    T, D = x.shape
    K, n = len(c['c0']), len(off)
    d = [dev(np.zeros(D) if shift is None else shift)] + [dev(c[k]) for k in ('A', 'B', 'c0', 'lw', 'ls', 'lr')]
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    ids, lp, nsw = _outputs(T, n, fill)
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    need = lib.abn_hmm_viterbi_ws_bytes(n, max(1, int(np.max(lens))), K, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    args = [p(x), T, D, p(off_d), p(len_d), n] + [p(t) for t in d[:4]] + [p(t) for t in d[4:]] + [K, p(ids), p(lp), p(nsw), p(ng),
                                                                                                 p(ws), need, _lib.stream()]
    rc = lib.abnx_hmm_viterbi_dur(*(args + [S])) if new else lib.abn_hmm_viterbi(*args)
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(ids), host(lp), host(nsw), host(ng)


def raw_km(x, m, b, off, lens, penalty, S, shift=None, new=True, fill=-7):
    """(ids, objective, n_switch) host arrays of abnx_kmeans_viterbi_dur (new=False: abn_kmeans_viterbi, S ignored)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    x = dev(x)
    T, D = x.shape
    K, n = len(b), len(off)
    sh, md, bd = dev(np.zeros(D) if shift is None else shift), dev(m), dev(b)
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    ids, obj, nsw = _outputs(T, n, fill)
    need = lib.abn_kmeans_viterbi_ws_bytes(n, max(1, int(np.max(lens))), K, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    args = [p(x), T, D, p(off_d), p(len_d), n, p(sh), p(md), p(bd), K, float(units_np.score_penalty(penalty)), p(ids), p(obj), p(nsw),
            p(ws), need, _lib.stream()]
    rc = lib.abnx_kmeans_viterbi_dur(*(args + [S])) if new else lib.abn_kmeans_viterbi(*args)
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(ids), host(obj), host(nsw)


# ---- exact cases ---------------------------------------------------------------------------------------------------------------
def plant(x, s, o):
    """Makes the 300 frames from row o three runs of one frame each, with unit boundaries at PLANTED: rows of x whose best
    unit wins by a clear margin and differs between neighbours.  With S >= 2 the forced run from frame 127 straddles the edge
    of the 128-frame block, and the traceback, which reaches frame 126 at the start of a 64-frame round, finds the cleared
    bit of the run from frame 62 at frame 61 + S >= 63 and the run's first frame in the NEXT round.  False: no such rows."""
    top = np.sort(s, axis=1)
    margin = top[:, -1] - (top[:, -2] if s.shape[1] > 1 else -np.inf)
    best = np.argmax(s, axis=1)
    for least in (2.0, 1.0, 0.5):
        rows = []
        for r in np.flatnonzero(margin >= least):
            if not rows or best[r] != best[rows[-1]]:
                rows.append(int(r))
            if len(rows) == 3:
                break
        if len(rows) == 3:
            break
    if len(rows) < 3:
        return False
    xa, sa = x[rows].copy(), s[rows].copy()
    for j, (lo, hi) in enumerate(((0, PLANTED[0]), PLANTED, (PLANTED[1], 300))):
        x[o + lo:o + hi], s[o + lo:o + hi] = xa[j], sa[j]
    return True


def starts(ids):
    """The first frames of the runs of ids (BAD frames taken out first; positions among the good frames)."""
    a = np.asarray(ids)
    a = a[a >= 0]
    return set((np.flatnonzero(a[1:] != a[:-1]) + 1).tolist())


def hmm_case(K, D, S, seed, n_dead=0):
    from test_gpu_hmm_vit import exact_case
    lens = lengths_for(S)
    off, T = layout(lens)
    c = exact_case(T, K, D, seed, n_dead=n_dead)
    planted = plant(c['x'], c['s'], int(off[-1]))
    return c, off, lens, T, planted


def km_case(K, D, S, seed):
    lens = lengths_for(S)
    off, T = layout(lens)
    x, m, b, s = units_np.exact_case(T, K, D, seed)
    planted = plant(x, s, int(off[-1]))
    return (x, m, b, s), off, lens, T, planted


def check_runs(ids, off, lens, S):
    for o, n in zip(off, lens):
        assert vit_dur_np.run_lengths_ok(ids[o:o + n], S), (o, n, S)


def check_hmm(c, off, lens, S, good=None, fill=-7):
    T = c['x'].shape[0]
    good = np.ones(T, dtype=bool) if good is None else good
    ref = vit_dur_np.viterbi(c['s'], good, off, lens, c['lw'], c['ls'], c['lr'], S)
    got = raw_hmm(c, off, lens, S, fill=fill)
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    assert np.array_equal(got[0][inside], ref[0][inside]), np.flatnonzero(inside & (got[0] != ref[0]))[:10]
    if fill is not None:
        assert (got[0][~inside] == fill).all()
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].dtype == np.int32
    check_runs(got[0], off, lens, S)
    return got


def check_km(case, off, lens, S, penalty, good=None, fill=-7):
    x, m, b, s = case
    T = x.shape[0]
    good = np.ones(T, dtype=bool) if good is None else good
    tables = vit_dur_np.kmeans_tables(len(b), units_np.score_penalty(penalty))
    ref = vit_dur_np.viterbi(s, good, off, lens, *tables, S)
    got = raw_km(x, m, b, off, lens, penalty, S, fill=fill)
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    assert np.array_equal(got[0][inside], ref[0][inside]), np.flatnonzero(inside & (got[0] != ref[0]))[:10]
    if fill is not None:
        assert (got[0][~inside] == fill).all()
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32
    check_runs(got[0], off, lens, S)
    return got


def check_planted(ids, off, K, planted):
    """The planted utterance was decoded with boundaries exactly where they were planted."""
    assert planted == (K > 1)
    if planted:
        assert set(PLANTED) <= starts(ids[off[-1]:off[-1] + 300])


# ---- a: exact equality -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('S', SS)
@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_hmm_exact_inputs_equal_the_restatement(K, D, S):
    c, off, lens, T, planted = hmm_case(K, D, S, seed=1000 * S + 100 * K + D)
    ids, lp, nsw, ng = check_hmm(c, off, lens, S)
    assert np.array_equal(ng, lens)
    check_planted(ids, off, K, planted)


@pytest.mark.parametrize('S', SS)
@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_kmeans_exact_inputs_equal_the_restatement(K, D, S):
    case, off, lens, T, planted = km_case(K, D, S, seed=1000 * S + 100 * K + D)
    for penalty in (0.0, 3.0):
        ids, obj, nsw = check_km(case, off, lens, S, penalty)
    check_planted(ids, off, K, planted)


def test_exact_inputs_at_the_largest_k_and_the_largest_minimum():
    from abnet3_amd import hmm, kmeans
    from test_gpu_hmm_vit import exact_case
    assert hmm.max_k() == 4096 and kmeans.viterbi_max_k() == 4096
    check_hmm(exact_case(130, 4096, 8, seed=7), [0], [130], 8)
    check_km(units_np.exact_case(130, 4096, 8, seed=7), [0], [130], 8, 3.0)


def test_hmm_exact_inputs_with_components_of_weight_zero():
    c, off, lens, T, _ = hmm_case(129, 16, 3, seed=129, n_dead=43)
    c['c0'][np.isneginf(c['lw'])] += 64.0                      # the dead components have by far the largest emissions
    c['s'] = (c['s'].astype(np.float64) + np.where(np.isneginf(c['lw']), 64.0, 0.0)).astype(np.float32)
    ids, lp, _, _ = check_hmm(c, off, lens, 3)
    assert np.isfinite(lp).all() and not np.isneginf(c['lw'])[ids[ids >= 0]].any()


# ---- b: S = 1 through the new entries is the old entries, bit for bit ------------------------------------------------------------
def float_hmm(K, seed, lens=None):
    from test_gpu_hmm_vit import Scores, recipe
    rng = np.random.default_rng(seed)
    lens = rng.integers(200, 401, size=6) if lens is None else lens
    x, shift, w, m, v = recipe(K, 40, lens, seed=1000 + seed, run_len=7)
    return lens, x, shift, w, Scores(x, shift, w, m, v)


def float_km(K, seed):
    rng = np.random.default_rng(seed)
    D = 40
    lens = rng.integers(200, 401, size=6)
    T = int(lens.sum())
    centres = rng.normal(size=(K, D))
    lab = np.repeat(rng.integers(0, K, size=T // 7 + 1), 7)[:T]
    x = (centres[lab] + 0.7 * rng.normal(size=(T, D))).astype(np.float32)
    xc, badrow, shift = kmeans_np.prepare(x)
    m, b = kmeans_np.tables(centres - shift.astype(np.float64) + 0.05 * rng.normal(size=(K, D)))
    s64, E = kmeans_np.scores(xc, badrow, m, b)
    assert not badrow.any()
    return lens, x, shift, m, b, s64, E


@pytest.fixture(scope='module')
def float_cases():
    cache = {}

    def get(kind, K):
        if (kind, K) not in cache:
            cache[kind, K] = float_hmm(K, K) if kind == 'hmm' else float_km(K, K)
        return cache[kind, K]
    return get


@pytest.mark.parametrize('K', [5, 129, 300])
def test_minimum_of_one_through_the_new_entries_is_the_old_entries_bit_for_bit(float_cases, K):
    bits = dirty_memory.bits
    # exact inputs, every length
    c, off, lens, T, _ = hmm_case(K, 40, 1, seed=K)
    new, old = raw_hmm(c, off, lens, 1), raw_hmm(c, off, lens, 1, new=False)
    assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(new, old))
    (x, m, b, s), off, lens, T, _ = km_case(K, 40, 1, seed=K)
    for penalty in (0.0, 3.0):
        new, old = raw_km(x, m, b, off, lens, penalty, 1), raw_km(x, m, b, off, lens, penalty, 1, new=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(new, old))
    # float data
    if K == 5:
        return
    lens, x, shift, w, sc = float_cases('hmm', K)
    off = np.cumsum(lens) - lens
    for stay in (0.0, 0.9):
        lw, ls, lr = hmm_vit_np.tables(w, stay)
        c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, lw=lw, ls=ls, lr=lr)
        new, old = raw_hmm(c, off, lens, 1, shift=shift), raw_hmm(c, off, lens, 1, shift=shift, new=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(new, old)) and new[2].sum() > 0
    lens, x, shift, m, b, s64, E = float_cases('km', K)
    off = np.cumsum(lens) - lens
    for penalty in (0.0, 3.0, 20.0):
        new = raw_km(x, m, b, off, lens, penalty, 1, shift=shift)
        old = raw_km(x, m, b, off, lens, penalty, 1, shift=shift, new=False)
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(new, old)) and new[2].sum() > 0


# ---- c: BAD frames -----------------------------------------------------------------------------------------------------------
def bad_rows(off, lens):
    """BAD frames inside the forced runs planted at frames 62 and 127 of the last utterance -- at the block edge, and a
    stretch of 70 that makes the forced run span more than one 64-frame round of the traceback --, first and last frames,
    the frames around the 128-frame block edge, and one utterance that is all BAD."""
    T = int(off[-1] + lens[-1] + 2)
    bad = np.zeros(T, dtype=bool)
    o = int(off[-1])
    bad[o + 63] = bad[o + 127] = bad[o + 128] = True
    bad[o + 130:o + 200] = True
    bad[o] = bad[o + 299] = True
    u300 = len(lens) - 2                                        # the other 300-frame utterance: block edges, first, last
    bad[off[u300] + np.array([0, 127, 128, 255, 256, 299])] = True
    u64 = list(lens).index(64)
    bad[off[u64]:off[u64] + 64] = True                          # all BAD
    u129 = list(lens).index(129)
    bad[off[u129] + 128] = True                                 # the only frame of its second block
    return bad


@pytest.mark.parametrize('S', SS)
def test_bad_frames_with_exact_inputs_equal_the_restatement(S):
    for K, D in ((5, 3), (129, 40)):
        c, off, lens, T, planted = hmm_case(K, D, S, seed=33 + S)
        bad = bad_rows(off, lens)
        c['x'][bad] = np.nan
        c['x'][off[-1] + 128, 1:] = 0.0                          # one NaN entry is enough
        c['x'][off[-1]] = np.inf
        ids, lp, nsw, ng = check_hmm(c, off, lens, S, good=~bad)
        u64 = list(lens).index(64)
        assert (ids[bad] == -1).all() and lp[u64] == 0.0 and nsw[u64] == 0 and ng[u64] == 0 and ng[-1] == 300 - 75
        assert planted and len(starts(ids[off[-1]:off[-1] + 300])) >= 2
        (x, m, b, s), off, lens, T, planted = km_case(K, D, S, seed=33 + S)
        x[bad] = np.nan
        x[off[-1]] = np.inf
        ids, obj, nsw = check_km((x, m, b, s), off, lens, S, 3.0, good=~bad)
        assert (ids[bad] == -1).all() and obj[u64] == 0.0 and nsw[u64] == 0
        assert planted and len(starts(ids[off[-1]:off[-1] + 300])) >= 2


# ---- d: float data against the float64 optimum ---------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [37, 300])
def test_hmm_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K):
    lens, x, shift, w, sc = float_cases('hmm', K)
    off = np.cumsum(lens) - lens
    assert not sc.bad.any()
    for stay in (0.5, 0.9, 0.99):
        t32 = hmm_vit_np.tables(w, stay)
        lmax = hmm_vit_np.table_max(*t32)
        c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, lw=t32[0], ls=t32[1], lr=t32[2])
        for S in SS:
            ids, lp, nsw, ng = raw_hmm(c, off, lens, S, shift=shift)
            assert np.array_equal(ng, lens)
            check_runs(ids, off, lens, S)
            # the maximal runs of the ids are the path's segments where re-entering a unit never beats staying in it
            runs_are_segments = bool((S * t32[1].astype(np.float64) >= t32[2].astype(np.float64)).all())
            assert runs_are_segments or stay == 0.5
            for u, (o, n) in enumerate(zip(off, lens)):
                sl = slice(o, o + n)
                good = np.ones(n, dtype=bool)
                opt = vit_dur_np.optimum_f64(sc.s64[sl], good, *t32, S)
                allow = 2.0 * n * vit_dur_np.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax, S)
                j64 = vit_dur_np.J_runs(sc.s64[sl], ids[sl], good, *t32, S)
                print('K %d stay %g S %d utt %d: optimum %.6f J_runs(device ids) %.6f device log_prob %.6f allowance %.3g switches %d'
                      % (K, stay, S, u, opt, j64, lp[u], allow, nsw[u]))
                if runs_are_segments:
                    assert opt - j64 <= allow and j64 <= opt + 1e-9 * (abs(opt) + 1.0)
                assert abs(lp[u] - opt) <= allow
                assert nsw[u] == hmm_vit_np.switches(ids[sl])


@pytest.mark.parametrize('K', [37, 300])
def test_kmeans_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K):
    lens, x, shift, m, b, s64, E = float_cases('km', K)
    off = np.cumsum(lens) - lens
    for penalty in (0.0, 3.0, 20.0):
        p = float(units_np.score_penalty(penalty))
        tables = vit_dur_np.kmeans_tables(K, p)
        for S in SS:
            ids, obj, nsw = raw_km(x, m, b, off, lens, penalty, S, shift=shift)
            check_runs(ids, off, lens, S)
            for u, (o, n) in enumerate(zip(off, lens)):
                sl = slice(o, o + n)
                good = np.ones(n, dtype=bool)
                opt = vit_dur_np.optimum_f64(s64[sl], good, *tables, S)
                allow = 2.0 * n * vit_dur_np.delta(E[sl], np.abs(s64[sl]).max() + E[sl].max(), p, S)
                j64 = vit_dur_np.J_runs(s64[sl], ids[sl], good, *tables, S)
                print('K %d penalty %g S %d utt %d: optimum %.6f J_runs(device ids) %.6f device objective %.6f allowance %.3g switches %d'
                      % (K, penalty, S, u, opt, j64, obj[u], allow, nsw[u]))
                assert opt - j64 <= allow and j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (ls = 0: the runs are the segments)
                assert abs(obj[u] - opt) <= allow
                assert nsw[u] == units_np.switches(ids[sl])


# ---- f: determinism and isolation ----------------------------------------------------------------------------------------------
def test_two_calls_are_bit_identical_rows_outside_are_untouched_and_an_utterance_does_not_see_its_neighbours():
    from test_gpu_hmm_vit import recipe
    rng = np.random.default_rng(8)
    lens = np.concatenate([rng.integers(1, 60, size=597), [300, 129, 128]])        # 600: more utterances than workgroups
    rng.shuffle(lens)
    off, T = layout(lens, gap=3)
    K, D, S = 200, 40, 3
    x, shift, w, m, v = recipe(K, D, [T], seed=8, run_len=6)
    A, B, _ = gmm_np.tables(w, m, v)
    lw, ls, lr = hmm_vit_np.tables(w, 0.9)
    c = dict(x=x, A=A, B=B, c0=hmm_np.emission_offsets(m, v), lw=lw, ls=ls, lr=lr)
    mk, bk = kmeans_np.tables(rng.normal(size=(K, D)))
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    u = int(np.argmax(lens))
    sl = slice(off[u], off[u] + lens[u])
    bits = dirty_memory.bits
    for run, alone in ((lambda: raw_hmm(c, off, lens, S, shift=shift, fill=-100000),
                        lambda: raw_hmm(dict(c, x=x[sl]), [0], [lens[u]], S, shift=shift)),
                       (lambda: raw_km(x, mk, bk, off, lens, 2.0, S, shift=shift, fill=-100000),
                        lambda: raw_km(x[sl], mk, bk, [0], [lens[u]], 2.0, S, shift=shift))):
        a, b = run(), run()
        assert all(np.array_equal(bits(p), bits(q)) for p, q in zip(a, b))
        assert (a[0][~inside] == -100000).all() and (~inside).sum() >= 3 * 601
        assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()
        check_runs(a[0], off, lens, S)
        one = alone()                                           # a grid of one workgroup, no neighbours
        assert np.array_equal(one[0], a[0][sl]) and all(bits(p)[0] == bits(q)[u] for p, q in zip(one[1:], a[1:]))


# ---- g: dirty memory ---------------------------------------------------------------------------------------------------------
def test_every_next_symbol_is_a_dirty_memory_case_or_the_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert _lib.load().abnx_viterbi_dur_max() == 8


@pytest.mark.parametrize('K', [5, 129])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(K):
    """Both entries of DIRTY_CASES with ids, the per-utterance outputs and the workspace from torch.empty under the three
    patterns: the same bits (rows outside every utterance keep the pattern), and the 0xFF run equals the restatement."""
    from abnet3_amd import _lib
    S = 3
    c, off, lens, T, _ = hmm_case(K, 40, S, seed=K)
    case = km_case(K, 40, S, seed=K)[0]
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    bits = dirty_memory.bits
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                if byte == 0xFF:
                    h, k = check_hmm(c, off, lens, S, fill=None), check_km(case, off, lens, S, 3.0, fill=None)
                else:
                    h, k = raw_hmm(c, off, lens, S, fill=None), raw_km(*case[:3], off, lens, 3.0, S, fill=None)
            assert int(count) >= 9 and count.nbytes > 2 * T * 4          # ids, three or two outputs and the workspace, twice
            word = np.frombuffer(bytes([byte]) * 4, dtype=np.int32)[0]
            assert (h[0][~inside] == word).all() and (k[0][~inside] == word).all()
            outs[byte] = [h[0][inside]] + list(h[1:]) + [k[0][inside]] + list(k[1:])
    assert set(old_calls) <= {'abn_hmm_viterbi_ws_bytes', 'abn_kmeans_viterbi_ws_bytes', 'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs[byte], outs[0x00])), hex(byte)


# ---- h: the public surface -------------------------------------------------------------------------------------------------------
def test_min_duration_through_segment_decode_quantize_and_the_command_lines(tmp_path):
    from abnet3_amd import gmm, hmm, kmeans, tde
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=40, D=13, n_phones=4, noise=0.6)
    corpus = DeviceCorpus(feats, times)
    seconds = corpus.total / 100.0
    S = 3

    def figures(ids):
        return kmeans.bitrate(kmeans.unit_sequences(ids), seconds), sum(len(v) for v in tde.unit_boundaries(ids, times).values())

    q = kmeans.KMeansQuantizer(8, n_iter=10).fit(corpus)
    plain = q.segment(corpus, 1.0)
    obj1, nsw1 = q.last_objective_.copy(), q.last_n_switch_.copy()
    assert all(np.array_equal(a, b) for a, b in zip(q.segment(corpus, 1.0, min_duration=1).values(), plain.values()))
    assert np.array_equal(q.last_objective_, obj1)
    ids = q.segment(corpus, 1.0, min_duration=S)
    assert list(ids) == corpus.names and q.last_objective_.shape == obj1.shape and q.last_n_switch_.dtype == np.int32
    for i, k in enumerate(corpus.names):
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],) and vit_dur_np.run_lengths_ok(ids[k], S)
        assert q.last_n_switch_[i] == units_np.switches(ids[k])
    assert (q.last_objective_ <= obj1 + 1e-3).all()                     # ls = 0: fewer paths, no greater objective
    assert not all(vit_dur_np.run_lengths_ok(plain[k], S) for k in plain), 'the planted corpus has no short unit to remove'
    rate, nb = figures(ids)
    rate1, nb1 = figures(plain)
    assert 0.0 < rate <= rate1 and nb <= nb1 and nb == int(q.last_n_switch_.sum())
    assert all(np.array_equal(a, b) for a, b in zip(q.predict(corpus, penalty=1.0, min_duration=S).values(), ids.values()))
    quant = q.quantize(corpus, penalty=1.0, min_duration=S)
    flat = np.concatenate([ids[k] for k in corpus.names])
    assert isinstance(quant, DeviceCorpus) and quant.names == corpus.names
    assert np.array_equal(host(quant.table), host(q.device_tables(quant.table.device)[3])[flat])
    one = corpus.names[0]
    alone = q.segment(dev(feats[one]), 1.0, min_duration=S)                        # a table: ONE utterance
    assert isinstance(alone, torch.Tensor) and np.array_equal(host(alone), ids[one])

    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    h = hmm.StickyHmmPosteriorgram(g, 0.8)
    hplain = h.decode(corpus)
    lp1 = h.last_log_prob_.copy()
    assert all(np.array_equal(a, b) for a, b in zip(h.decode(corpus, min_duration=1).values(), hplain.values()))
    assert np.array_equal(h.last_log_prob_, lp1)
    hids = h.decode(corpus, min_duration=S)
    assert list(hids) == corpus.names and h.last_log_prob_.dtype == np.float64 and h.last_n_good_.tolist() == [corpus.length[k] for k in corpus.names]
    for i, k in enumerate(corpus.names):
        assert vit_dur_np.run_lengths_ok(hids[k], S) and h.last_n_switch_[i] == units_np.switches(hids[k])
    rate, nb = figures(hids)
    rate1, nb1 = figures(hplain)
    assert 0.0 < rate <= rate1 and nb <= nb1
    hq = h.quantize(corpus, min_duration=S)
    hflat = np.concatenate([hids[k] for k in corpus.names])
    assert isinstance(hq, DeviceCorpus) and np.array_equal(host(hq.table), g.means_.astype(np.float32)[hflat])

    # the command lines
    fpath = str(tmp_path / 'feats.npz')
    np.savez(fpath, **feats)
    kpath, hpath = str(tmp_path / 'km.npz'), str(tmp_path / 'hmm.npz')
    q.save(kpath)
    h.save(hpath)
    for main, argv, ref in ((kmeans.main, ['transform', kpath, fpath, str(tmp_path / 'k.npz'), '--penalty', '1.0', '--min-duration', str(S)], ids),
                            (hmm.main, ['decode', hpath, fpath, str(tmp_path / 'h.npz'), '--min-duration', str(S)], hids)):
        assert main(argv) == 0
        with np.load(argv[3]) as z:
            assert sorted(z.files) == sorted(ref) and all(np.array_equal(z[k], ref[k]) for k in ref)
