"""abn_hmm_viterbi and StickyHmmPosteriorgram.decode / quantize on the MI355X against tests/hmm_vit_np.py.

Exact inputs: integer frames in [-3, 3], shift 0, A integer in [-2, 2], B = -0.5, c0 and the three log tables multiples of
1/8 -- every fp32 operation of the score GEMM and of the recurrence is then exact, ties are plentiful, and ids, log_prob,
n_switch and n_good must EQUAL the restatement's.  Random float data is compared through the float64 log joint with the
allowance hmm_vit_np's docstring derives (2 n_good delta)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_np  # noqa: E402
import hmm_vit_np  # noqa: E402
import units_np  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
KS, DS = (1, 5, 64, 65, 128, 129, 257, 300), (1, 15, 16, 39, 127)
STAYS = (0.0, 0.5, 0.9, 0.99)


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return None if t is None else t.detach().cpu().numpy()


def layout(lengths, gap=2):
    """Offsets of utterances laid out in the given order with `gap` rows outside every utterance between them."""
    off, o = [], gap
    for n in lengths:
        off.append(o)
        o += n + gap
    return np.array(off, dtype=np.int64), o


def exact_case(T, K, D, seed, n_dead=0):
    """dict(x, A, B, c0, lw, ls, lr, s): integer frames and tables in eighths, the float32 scores s exact."""
    rng = np.random.default_rng(seed)
    x = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    A = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = (rng.integers(-16, 17, size=K) / 8.0).astype(np.float32)
    ls = (-rng.integers(0, 9, size=K) / 8.0).astype(np.float32)
    lr = (ls - rng.integers(0, 25, size=K) / 8.0).astype(np.float32)
    lw = (-rng.integers(0, 41, size=K) / 8.0).astype(np.float32)
    if n_dead:
        dead = rng.choice(K, size=n_dead, replace=False)
        lw[dead], lr[dead] = -np.inf, -np.inf
    x64, A64 = x.astype(np.float64), A.astype(np.float64)
    s64 = x64 @ A64.T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64) and (lr <= ls).all()
    return dict(x=x, A=A, B=B, c0=c0, lw=lw, ls=ls, lr=lr, s=s)


def run(c, off, lens, ids=None, shift=None, want_log_prob=True):
    from abnet3_amd import hmm
    D = c['x'].shape[1]
    shift = np.zeros(D, dtype=np.float32) if shift is None else shift
    out = hmm.viterbi(dev(c['x']), off, lens, dev(shift), dev(c['A']), dev(c['B']), dev(c['c0']), dev(c['lw']), dev(c['ls']),
                      dev(c['lr']), ids=ids, want_log_prob=want_log_prob)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


def prefilled(T):
    return torch.full((T,), -7, dtype=torch.int32, device='cuda')


def check_exact(c, off, lens):
    T = c['x'].shape[0]
    ref = hmm_vit_np.viterbi(c['s'], np.ones(T, dtype=bool), off, lens, c['lw'], c['ls'], c['lr'])
    got = run(c, off, lens, ids=prefilled(T))
    assert np.array_equal(got[0], ref[0]), np.flatnonzero(got[0] != ref[0])[:10]
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3])
    assert got[0].dtype == np.int32 and got[1].dtype == np.float64 and got[2].dtype == np.int32 and got[3].dtype == np.int32
    return got


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_exact_inputs_equal_the_restatement(K, D):
    off, T = layout(LENGTHS)
    c = exact_case(T, K, D, seed=100 * K + D)
    ids, lp, nsw, ng = check_exact(c, off, LENGTHS)
    assert np.array_equal(ng, LENGTHS)
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, LENGTHS):
        inside[o:o + n] = True
    assert (ids[~inside] == -7).all() and (ids[inside] >= 0).all() and (ids[inside] < K).all()
    # the same utterances handed over in another order: the same rows get the same ids
    perm = np.random.default_rng(K + D).permutation(len(LENGTHS))
    ids2, lp2, nsw2, ng2 = run(c, off[perm], np.array(LENGTHS)[perm], ids=prefilled(T))
    assert np.array_equal(ids2, ids) and np.array_equal(lp2, lp[perm]) and np.array_equal(nsw2, nsw[perm])
    assert np.array_equal(ng2, ng[perm])


def test_exact_inputs_at_the_largest_k():
    from abnet3_amd import hmm
    c = exact_case(130, hmm.max_k(), 8, seed=7)
    check_exact(c, [0], [130])


@pytest.mark.parametrize('K', [5, 129, 300])
def test_exact_inputs_with_components_of_weight_zero(K):
    lens = (129, 64, 1, 300)
    off, T = layout(lens)
    c = exact_case(T, K, 16, seed=K, n_dead=max(1, K // 3))
    c['c0'][np.isneginf(c['lw'])] += 64.0                     # the dead components have by far the largest emissions
    c['s'] = (c['s'].astype(np.float64) + np.where(np.isneginf(c['lw']), 64.0, 0.0)).astype(np.float32)
    ids, lp, _, _ = check_exact(c, off, lens)
    assert np.isfinite(lp).all() and not np.isneginf(c['lw'])[ids[ids >= 0]].any()


def test_both_max_product_chains_back_to_back_equal_their_restatements():
    """The k-means and the HMM max-product chain (one workspace geometry, utt_chain.h's) on one corpus, launched back to
    back on one stream with no synchronisation between: K = 130 puts both slabs in the workspace (ks = 256) with the same stay words per
    frame, the k-means regions carry 8 bytes of tail and the HMM's none, 600 utterances are more than the workgroups, and
    some are exactly 128 and 129 frames long.  Each must equal its numpy restatement bit for bit."""
    from abnet3_amd import hmm, kmeans
    K, D = 130, 8
    rng = np.random.default_rng(130)
    lens = np.concatenate([[1, 128, 129, 300, 128, 129], rng.integers(1, 48, size=590), [300, 257, 128, 129]])
    rng.shuffle(lens)
    off, T = layout(lens)
    c = exact_case(T, K, D, seed=100 * K + D)
    x, m, b, s = units_np.exact_case(T, K, D, seed=100 * K + D)
    good = np.ones(T, dtype=bool)
    ref_k = units_np.viterbi(s, good, off, lens, units_np.score_penalty(3.0))
    ref_h = hmm_vit_np.viterbi(c['s'], good, off, lens, c['lw'], c['ls'], c['lr'])
    shift = dev(np.zeros(D, dtype=np.float32))
    args_k = (dev(x), off, lens, shift, dev(m), dev(b), 3.0)
    args_h = (dev(c['x']), off, lens, shift) + tuple(dev(c[k]) for k in ('A', 'B', 'c0', 'lw', 'ls', 'lr'))
    torch.cuda.synchronize()
    for _ in range(2):                                                     # (the second round: each after the other's launch)
        got_k = kmeans.viterbi(*args_k, ids=prefilled(T), want_objective=True)
        got_h = hmm.viterbi(*args_h, ids=prefilled(T))
        torch.cuda.synchronize()
        for got, ref in ((got_k, ref_k), (got_h, ref_h)):
            assert len(got) == len(ref)
            for g, r in zip(got, ref):
                assert np.array_equal(host(g), r), np.flatnonzero(host(g) != r)[:10]


# ---- 2: stay = 0 against the mixture -------------------------------------------------------------------------------------
def recipe(K, D, lens, seed, run_len=1):
    """Centres 0.35 N(0, 1), unit noise, variances in [1, 1.2], Dirichlet(5) weights: frames in label runs of run_len.
    (x float32, shift float32, w, centred means m, variances v)"""
    rng = np.random.default_rng(seed)
    T = int(np.sum(lens))
    centres = 0.35 * rng.normal(size=(K, D))
    lab = np.repeat(rng.integers(0, K, size=T // run_len + 1), run_len)[:T]
    x = (centres[lab] + rng.normal(size=(T, D))).astype(np.float32)
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    m = centres - shift.astype(np.float64)
    v = rng.uniform(1.0, 1.2, size=(K, D))
    w = rng.dirichlet(np.full(K, 5.0))
    return x, shift, w, m, v


def mixture(shift, w, m, v):
    from abnet3_amd.gmm import GmmPosteriorgram
    g = GmmPosteriorgram(len(w))
    g.weights_, g.means_, g.variances_ = w.astype(np.float64), m + shift.astype(np.float64), v.astype(np.float64)
    g.shift_, g.gv_ = shift, np.ones(m.shape[1])
    return g


class Scores(object):
    """The float64 emission scores of a recipe under the fp32 device tables, and their forward bound."""

    def __init__(self, x, shift, w, m, v):
        self.xc, self.bad = gmm_np.centre(x, shift)
        self.A, self.B, _ = gmm_np.tables(w, m, v)
        self.c0 = hmm_np.emission_offsets(m, v)
        self.s64 = gmm_np.scores(self.xc, self.bad, self.A, self.B, self.c0, np.float64)
        self.scale = gmm_np.score_scale(self.xc, self.bad, self.A, self.B, self.c0)
        self.E = hmm_vit_np.score_bound(self.scale, x.shape[1]).max(axis=1)         # per frame


@pytest.mark.parametrize('K,D', [(37, 40), (129, 100)])
def test_zero_stay_gives_the_mixtures_hard_assignment(K, D):
    from abnet3_amd import hmm
    T = 900
    x, shift, w, m, v = recipe(K, D, [T], seed=K + D)
    g = mixture(shift, w, m, v)
    table = dev(x)
    ids = host(hmm.StickyHmmPosteriorgram(g, stay=0.0).decode(table))
    post = host(g.transform(table))
    sc = Scores(x, shift, w, m, v)
    assert not sc.bad.any() and ids.shape == (T,) and ids.dtype == np.int32
    lw = hmm_vit_np.tables(w, 0.0)[0].astype(np.float64)
    tot = sc.s64 + lw[None, :]
    top = np.sort(tot, axis=1)
    margin = top[:, -1] - top[:, -2]
    # a frame's bound covers both routes: the score tile with c0 (the HMM) or c = c0 + log w (the mixture) as the last
    # term, and the HMM's one rounded addition of lw
    bound = (hmm_vit_np.score_bound(sc.scale + np.abs(lw)[None, :], D) + 2.0 * hmm_vit_np.U * (np.abs(sc.s64) + np.abs(lw)[None, :])).max(axis=1)
    exempt = margin < 2.0 * bound
    print('K %d D %d: %d of %d frames under the margin (largest bound %.3g, smallest margin %.3g), %d ids differ'
          % (K, D, int(exempt.sum()), T, bound.max(), margin.min(), int((ids != post.argmax(axis=1)).sum())))
    assert exempt.sum() <= T // 100
    assert np.array_equal(ids[~exempt], post.argmax(axis=1)[~exempt])
    assert np.array_equal(ids[~exempt], tot.argmax(axis=1)[~exempt])


# ---- 3: random float data against the float64 optimum ----------------------------------------------------------------------
@pytest.fixture(scope='module')
def float_cases():
    cache = {}

    def get(K):
        if K not in cache:
            rng = np.random.default_rng(K)
            lens = rng.integers(200, 401, size=12)
            x, shift, w, m, v = recipe(K, 40, lens, seed=1000 + K, run_len=7)
            cache[K] = (lens, x, shift, w, Scores(x, shift, w, m, v))
        return cache[K]
    return get


def float_run(case, stay):
    lens, x, shift, w, sc = case
    lw, ls, lr = hmm_vit_np.tables(w, stay)
    c = dict(x=x, A=sc.A, B=sc.B, c0=sc.c0, lw=lw, ls=ls, lr=lr)
    return run(c, np.cumsum(lens) - lens, lens, shift=shift), (lw, ls, lr)


@pytest.mark.parametrize('K', [37, 300])
def test_float_data_is_within_the_derived_allowance_of_the_float64_optimum(float_cases, K):
    case = float_cases(K)
    lens, x, shift, w, sc = case
    off = np.cumsum(lens) - lens
    assert not sc.bad.any()
    totals = []
    for stay in STAYS:
        (ids, lp, nsw, ng), t32 = float_run(case, stay)
        lmax = hmm_vit_np.table_max(*t32)
        assert np.array_equal(ng, lens)
        for u, (o, n) in enumerate(zip(off, lens)):
            sl = slice(o, o + n)
            good = np.ones(n, dtype=bool)
            opt = hmm_vit_np.optimum_f64(sc.s64[sl], good, *t32)
            allow = 2.0 * n * hmm_vit_np.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax)
            j64 = hmm_vit_np.J(sc.s64[sl], ids[sl], good, *t32)
            print('K %d stay %g utt %d: optimum %.6f J64(device ids) %.6f device log_prob %.6f allowance %.3g switches %d'
                  % (K, stay, u, opt, j64, lp[u], allow, nsw[u]))
            assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (the upper side: float64 rounding of the two sums only)
            assert abs(lp[u] - opt) <= allow
            assert nsw[u] == hmm_vit_np.switches(ids[sl])
        totals.append(int(nsw.sum()))
    print('K %d: switches over stay %s: %s' % (K, STAYS, totals))
    assert all(b <= a for a, b in zip(totals, totals[1:])), totals
    assert totals[-1] < totals[0]


# ---- 4: BAD frames ---------------------------------------------------------------------------------------------------------
def test_bad_frames_get_minus_one_and_the_chain_passes_over_them():
    lens = np.array([140, 5, 260, 3])
    K, D = 9, 12
    x, shift, w, m, v = recipe(K, D, lens, seed=21, run_len=5)
    off = np.cumsum(lens) - lens
    bad_rows = {0: [0, 70, 139], 1: [], 2: [127, 128, 200], 3: [0, 1, 2]}          # first / middle / last; block edges; all
    xb = x.copy()
    for u, rows in bad_rows.items():
        for j, r in enumerate(rows):
            xb[off[u] + r] = np.inf
            if j % 2:
                xb[off[u] + r] = x[off[u] + r]
                xb[off[u] + r, 3] = np.nan
    sc = Scores(xb, shift, w, m, v)
    flat = np.concatenate([off[u] + np.array(r, dtype=np.int64) for u, r in bad_rows.items()])
    assert sorted(np.flatnonzero(sc.bad)) == sorted(flat.tolist())
    for stay in (0.0, 0.9):
        lw, ls, lr = hmm_vit_np.tables(w, stay)
        c = dict(x=xb, A=sc.A, B=sc.B, c0=sc.c0, lw=lw, ls=ls, lr=lr)
        ids, lp, nsw, ng = run(c, off, lens, shift=shift)
        assert (ids[sc.bad] == -1).all() and (ids[~sc.bad] >= 0).all()
        assert ng.tolist() == [137, 5, 257, 0] and lp[3] == 0.0 and nsw[3] == 0
        # passed over: the table without the BAD rows gives the other rows' bits
        keep = np.flatnonzero(~sc.bad)
        lens2 = np.array([137, 5, 257])
        c2 = dict(c, x=xb[keep])
        ids2, lp2, nsw2, ng2 = run(c2, np.cumsum(lens2) - lens2, lens2, shift=shift)
        assert np.array_equal(ids2, ids[keep]) and np.array_equal(lp2, lp[:3]) and np.array_equal(nsw2, nsw[:3])
        assert np.array_equal(ng2, ng[:3])
        # and it equals the restatement run on the device's own good scores within the float allowance: here through the
        # exact relation instead -- the float32 restatement on the float64 scores rounded once has the same optimum up to
        # the allowance
        lmax = hmm_vit_np.table_max(lw, ls, lr)
        for u, (o, n) in enumerate(zip(off, lens)):
            sl = slice(o, o + n)
            good = ~sc.bad[sl]
            opt = hmm_vit_np.optimum_f64(sc.s64[sl], good, lw, ls, lr)
            ngood = int(good.sum())
            E = sc.E[sl][good] if ngood else np.zeros(1)
            smax = np.abs(sc.s64[sl][good]).max() + E.max() if ngood else 0.0
            allow = 2.0 * ngood * hmm_vit_np.delta(E, smax, lmax)
            assert abs(lp[u] - opt) <= allow and nsw[u] == hmm_vit_np.switches(ids[sl])
            if ngood:
                assert opt - allow <= hmm_vit_np.J(sc.s64[sl], ids[sl], good, lw, ls, lr) <= opt + 1e-9 * (abs(opt) + 1.0)


def test_bad_frames_with_exact_inputs_equal_the_restatement():
    lens = (140, 5, 260, 3)
    off, T = layout(lens)
    c = exact_case(T, 65, 15, seed=33)
    bad = np.zeros(T, dtype=bool)
    for u, rows in enumerate(([0, 70, 139], [], [127, 128, 200], [0, 1, 2])):
        bad[off[u] + np.array(rows, dtype=np.int64)] = True
    c['x'][bad] = np.nan
    c['x'][off[2] + 128, 1:] = 0.0                                                    # one NaN entry is enough
    c['x'][off[0]] = np.inf
    ref = hmm_vit_np.viterbi(c['s'], ~bad, off, lens, c['lw'], c['ls'], c['lr'])
    got = run(c, off, lens, ids=prefilled(T))
    for a, b in zip(got, ref):
        assert np.array_equal(a, b)
    assert (got[0][bad] == -1).all() and got[1][3] == 0.0 and got[2][3] == 0 and got[3][3] == 0


# ---- 5: slab and workspace reuse -------------------------------------------------------------------------------------------
def test_thousands_of_short_utterances_reuse_the_slabs():
    n = 3000
    rng = np.random.default_rng(4)
    lens = rng.integers(1, 4, size=n)
    off = 1 + 4 * np.arange(n, dtype=np.int64)
    T = 4 * n + 1
    c = exact_case(T, 5, 4, seed=4)
    ids, lp, nsw, ng = check_exact(c, off, lens)
    inside = np.zeros(T, dtype=bool)
    for o, k in zip(off, lens):
        inside[o:o + k] = True
    assert (ids[~inside] == -7).all() and (~inside).sum() >= n and nsw.max() > 0
    again = run(c, off, lens, ids=prefilled(T))
    assert all(np.array_equal(a, b) for a, b in zip((ids, lp, nsw, ng), again)) and again[1].tobytes() == lp.tobytes()
    only = run(c, off, lens, ids=prefilled(T), want_log_prob=False)
    assert np.array_equal(only[0], ids) and only[1] is None and only[2] is None and np.array_equal(only[3], ng)


def test_two_calls_are_bit_identical_and_other_rows_are_untouched():
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 400, size=300)
    off, T = layout(lens, gap=3)
    K, D = 200, 40
    x, shift, w, m, v = recipe(K, D, [T], seed=8, run_len=6)
    A, B, _ = gmm_np.tables(w, m, v)
    lw, ls, lr = hmm_vit_np.tables(w, 0.9)
    c = dict(x=x, A=A, B=B, c0=hmm_np.emission_offsets(m, v), lw=lw, ls=ls, lr=lr)
    sentinel = torch.arange(T, dtype=torch.int32, device='cuda') - 100000
    a = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    b = run(c, off, lens, ids=sentinel.clone(), shift=shift)
    assert all(np.array_equal(u, v) for u, v in zip(a, b)) and a[1].tobytes() == b[1].tobytes()
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    assert np.array_equal(a[0][~inside], host(sentinel)[~inside]) and (~inside).sum() >= 3 * 301
    assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()
    # an utterance alone gives the rows it gave among its neighbours
    u = int(np.argmax(lens))
    one = run(dict(c, x=x[off[u]:off[u] + lens[u]]), [0], [lens[u]], shift=shift)
    assert np.array_equal(one[0], a[0][off[u]:off[u] + lens[u]]) and one[1][0] == a[1][u] and one[2][0] == a[2][u]


def test_refused_utterances_and_refusals_at_the_raw_entry():
    """Straight at the library: a bad off / len, or a len beyond what the workspace was sized for, marks its utterance and
    touches nothing; the refusals return their codes before any launch."""
    from abnet3_amd import _lib
    lib = _lib.load()
    K, D, T = 5, 13, 400
    c = exact_case(T, K, D, seed=17)
    d = {k: dev(c[k]) for k in ('x', 'A', 'B', 'c0', 'lw', 'ls', 'lr')}
    d['shift'] = dev(np.zeros(D))
    off = np.array([0, -1, 10, T - 3, 30], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300], dtype=np.int32)          # fine, off < 0, len < 0, past the end, longer than the workspace holds
    ids = torch.full((T,), -7, dtype=torch.int32, device='cuda')
    lp = torch.zeros(5, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(5, dtype=torch.int32, device='cuda')
    ng = torch.zeros(5, dtype=torch.int32, device='cuda')
    need = lib.abn_hmm_viterbi_ws_bytes(5, 100, K, D)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    p = _lib.ptr

    def call(**kw):
        a = dict(x=p(d['x']), T=T, D=D, off=p(off_d), len=p(len_d), n=5, shift=p(d['shift']), A=p(d['A']), B=p(d['B']),
                 c0=p(d['c0']), lw=p(d['lw']), ls=p(d['ls']), lr=p(d['lr']), K=K, ids=p(ids), lp=p(lp), nsw=p(nsw), ng=p(ng),
                 ws=p(ws), bytes=need, stream=_lib.stream())
        a.update(kw)
        return lib.abn_hmm_viterbi(*a.values())
    assert call() == 0
    torch.cuda.synchronize()
    gids, glp, gnsw, gng = host(ids), host(lp), host(nsw), host(ng)
    assert list(gng) == [5, -1, -1, -1, -1] and list(gnsw[1:]) == [-1] * 4 and np.isfinite(glp[0]) and np.isnan(glp[1:]).all()
    assert (gids[5:] == -7).all()
    ref = hmm_vit_np.viterbi(c['s'], np.ones(T, dtype=bool), [0], [5], c['lw'], c['ls'], c['lr'])
    assert np.array_equal(gids[:5], ref[0][:5]) and glp[0] == ref[1][0] and gnsw[0] == ref[2][0]
    before = ids.clone()
    assert call(lp=None, nsw=None, ng=None) == 0                    # the three per-utterance outputs may be NULL
    torch.cuda.synchronize()
    assert torch.equal(ids, before)
    assert call(ids=None) == _lib.E_ARG and call(lw=None) == _lib.E_ARG and call(T=0) == _lib.E_ARG
    assert call(K=lib.abn_hmm_max_k() + 1) == _lib.E_UNSUPPORTED and call(D=lib.abn_gmm_max_d() + 1) == _lib.E_UNSUPPORTED
    assert call(bytes=5 * 128 * 128 * 4) == _lib.E_WORKSPACE and call(ws=None) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(ids, before)


# ---- 6: consistency with the sum-product kernel ----------------------------------------------------------------------------
@pytest.mark.parametrize('stay', [0.0, 0.9])
def test_log_prob_is_below_the_sum_product_likelihood(float_cases, stay):
    from abnet3_amd import hmm
    case = float_cases(37)
    lens, x, shift, w, sc = case
    off = np.cumsum(lens) - lens
    (ids, lp, nsw, ng), t32 = float_run(case, stay)
    _, ll, _, ng_fb = hmm.forward_backward(dev(x), off, lens, dev(shift), dev(sc.A), dev(sc.B), dev(sc.c0), dev(w.astype(np.float32)),
                                           stay, 'filter', want_stays=False)
    ll, ng_fb = host(ll), host(ng_fb)
    assert np.array_equal(ng, ng_fb)
    lmax = hmm_vit_np.table_max(*t32)
    for u, (o, n) in enumerate(zip(off, lens)):
        sl = slice(o, o + n)
        # both sides carry the score bound of every frame; the max-product side the rest of its delta, the sum-product
        # side test_gpu_hmm.py's chain term (K + 16) 2^-24 per frame and 2 x 2^-24 |m_t|
        allow = n * (hmm_vit_np.delta(sc.E[sl], np.abs(sc.s64[sl]).max() + sc.E[sl].max(), lmax) + sc.E[sl].max()
                     + (37 + 16) * hmm_vit_np.U + 2.0 * hmm_vit_np.U * np.abs(sc.s64[sl]).max())
        assert lp[u] <= ll[u] + allow, (u, lp[u], ll[u], allow)


# ---- 7: the public layer -----------------------------------------------------------------------------------------------------
def test_decode_and_quantize_of_a_corpus_and_downstream(tmp_path):
    from abnet3_amd import eskmeans, gmm, hmm, kmeans
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=40, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    h = hmm.StickyHmmPosteriorgram(g, 0.8)
    ids = h.decode(corpus)
    assert list(ids) == corpus.names and h.last_log_prob_.shape == (len(corpus.names),)
    assert h.last_log_prob_.dtype == np.float64 and h.last_n_switch_.dtype == np.int32 and h.last_n_good_.dtype == np.int32
    assert h.n_bad_ == 0 and h.last_n_good_.tolist() == [corpus.length[k] for k in corpus.names]
    for i, k in enumerate(corpus.names):
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],) and (ids[k] >= 0).all() and (ids[k] < 8).all()
        assert h.last_n_switch_[i] == hmm_vit_np.switches(ids[k])
    lp = h.last_log_prob_.copy()
    assert all(np.array_equal(a, c) for a, c in zip(h.decode(feats).values(), ids.values()))      # the dict form
    assert np.array_equal(h.last_log_prob_, lp)
    one = corpus.names[0]
    alone = h.decode(dev(feats[one]))                                                              # a table: ONE utterance
    assert isinstance(alone, torch.Tensor) and alone.dtype == torch.int32 and np.array_equal(host(alone), ids[one])
    assert h.last_log_prob_.shape == (1,) and h.last_log_prob_[0] == lp[0]
    # downstream: what KMeansQuantizer.segment's ids feed
    plain = hmm.StickyHmmPosteriorgram(g, 0.0).decode(corpus)
    seq, seq_plain = kmeans.unit_sequences(ids), kmeans.unit_sequences(plain)
    assert sum(len(v) for v in seq.values()) <= sum(len(v) for v in seq_plain.values())
    seconds = corpus.total / 100.0
    assert 0.0 < kmeans.bitrate(seq, seconds) < np.inf
    seg = kmeans.segments(ids)
    assert all(np.array_equal(seg[k][2], seq[k]) and int((seg[k][1] - seg[k][0]).sum()) == corpus.length[k] for k in ids)
    lm = eskmeans.landmarks_from_units(seg, {k: corpus.length[k] for k in corpus.names})
    assert set(lm) == set(corpus.names) and all(lm[k][0] == 0 and lm[k][-1] == corpus.length[k] for k in lm)
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
    path = str(tmp_path / 'hmm.npz')
    h.save(path)
    again = hmm.StickyHmmPosteriorgram.load(path).decode(corpus)
    assert all(np.array_equal(again[k], ids[k]) for k in ids)
    fpath, opath = str(tmp_path / 'feats.npz'), str(tmp_path / 'ids.npz')
    np.savez(fpath, **feats)
    assert hmm.main(['decode', path, fpath, opath]) == 0
    with np.load(opath) as z:
        assert sorted(z.files) == sorted(ids) and all(np.array_equal(z[k], ids[k]) and z[k].dtype == np.int32 for k in ids)
