"""abn_hmm_forward_backward_stats, abn_hmm_accumulate and StickyHmmPosteriorgram.fit on the MI355X against
tests/hmm_bw_np.py.

The error bars (all derived, none tuned):
* stay_k: tests/test_gpu_hmm.py's bar on `stays`, n_good expm1(2 S) with S the utterance's sum of eps_t + delta.  The
  terms rho ahat_p[k] e_t[k] are non-negative and every one carries the same relative error e^(+-2 S), so the bar on
  their sum bounds each component's share; the fp32 sum over a block adds at most 127 x 2^-24 relative, inside delta's
  K + 16 per frame.  sum_k stay_k against the kernel's own `stays`: both carry the bar.
* accumulate, the same fp32 `post` on both sides: a sum of n terms in any order is within (n - 1) u sum |terms| to first
  order; n = the frames of a range, + 1 for the product's rounding, + 1 for the first order:
  |err| <= (frames per range + 2) 2^-24 sum_t |g x~|.  The float64 sum over the ranges adds nothing at this scale.
* the kernel's sums against the all-float64 restatement: that bar plus sum_t allowed_gamma[t, k] |x~[t, col]| with
  test_gpu_hmm.py's bar on gamma, allowed_gamma = g64 expm1(2 S) + 2^-22.
* fit against the float64 EM of the restatement: max(2^-22, 4 x yardstick) of each array's largest magnitude, the
  yardstick being the float32 restatement's own distance from the float64 one after the same iterations (measured on
  the CPU inside the test).  Measured yardsticks, seed 0, 8 iterations: see test_fit_on_a_planted_corpus.
Each check prints the largest fraction of its bar that was reached (-s shows it).

Largest fractions seen on the MI355X: stay_k 2.9e-4 of its bar (K = 3, D = 1, rho = 0.9), sum_k stay_k against stays
1.6e-4; accumulate against float64 over the same table 0.077 (T = 129, K = 130, D = 100); the sums of the kernel's gamma
against the all-float64 restatement 1.5e-3 (K = 130, D = 5, rho = 0.999); on abn_gmm_posteriors' table the sums were
bit-equal to abn_gmm_mstep's.  fit after 8 iterations: the kernel's distance from the float64 EM was 0.03 - 0.2 of the
float32 restatement's own in the weights, means and variances, and 0.5 (seed 0) and 2.0 (seed 1) of it in the stay, where
one float32 step of the stay itself is 6.6e-8."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_bw_np  # noqa: E402
import hmm_np  # noqa: E402
from test_gpu_hmm import Case, FLOOR, U, dev, host, make_model  # noqa: E402

pytestmark = pytest.mark.gpu

LENS = (0, 1, 2, 127, 128, 129, 300)
OFF = (0, 0, 1, 8, 135, 263, 392)                         # rows 3 .. 7 belong to no utterance
T_ROWS = 700                                              # 692 rows of utterances and the gap, 8 rows behind the last utterance
BAD_ROWS = [2, 8, 262, 300] + list(range(392 + 128, 392 + 256))      # a last frame, a first frame, a last frame, the middle, a whole block
GRID = [(3, 1, 0.9), (130, 5, 0.999), (300, 40, 0.0), (513, 5, 0.9), (130, 40, 0.9), (3, 5, 0.0),
        (1025, 5, 0.9), (2049, 1, 0.999)]                 # the last two: 8 and 16 components per thread


def make_case(K, D):
    x, shift, w, m, v = make_model(T_ROWS, K, D, seed=7000 * K + D, zero_weight=1)
    x[2, 0], x[8, D - 1], x[262, 0], x[300, D // 2] = np.nan, np.inf, -np.inf, 3e19
    x[392 + 128:392 + 256, 0] = np.nan
    case = Case(x, shift, w, m, v, LENS)
    case.off = np.asarray(OFF, dtype=np.int64)
    assert list(np.flatnonzero(case.bad)) == BAD_ROWS and case.w32[1] == 0.0
    return case


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(K, D):
        if (K, D) not in cache:
            cache[(K, D)] = make_case(K, D)
        return cache[(K, D)]
    return get


def run_stats(case, rho, mode='smooth', off=None, lens=None, table=None):
    from abnet3_amd import hmm
    d = case.d
    post, ll, st, ng, sk = hmm.forward_backward(d['table'] if table is None else table, case.off if off is None else off,
                                                case.lens if lens is None else lens, d['shift'], d['A'], d['B'], d['c0'], d['w'],
                                                rho, mode, want_stay_k=True)
    torch.cuda.synchronize()
    return dict(post=post, loglik=ll, stays=st, n_good=ng, stay_k=sk)


def run_plain(case, rho, mode='smooth'):
    from abnet3_amd import hmm
    d = case.d
    post, ll, st, ng = hmm.forward_backward(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], d['w'], rho, mode)
    return dict(post=post, loglik=ll, stays=st, n_good=ng)


def reference_stay_k(case, rho):
    s64 = case.scores()['s64']
    return np.array([hmm_bw_np.forward_backward(s64[o:o + n], case.bad[o:o + n], case.w32, rho)['stay_k']
                     for o, n in zip(case.off, case.lens)])


def frames_per_range(T, K, n_ranges):
    """The host's grid (abn_gmm_accumulate's): frame blocks of 128 in at most n_ranges (0: 1024 / tiles, 256 at most) ranges."""
    tiles, fblocks = (K + 127) // 128, (T + 127) // 128
    r = n_ranges if n_ranges > 0 else (1024 + tiles - 1) // tiles
    r = min(r, 256, fblocks)
    return 128 * ((fblocks + r - 1) // r)


def augment_elementwise(x, shift, dtype=np.float64):
    """[xc | xc^2 | 1] with the device's rule per ELEMENT: an entry whose fp32 xc^2 is not finite is 0 in both blocks."""
    with np.errstate(all='ignore'):
        xc = (np.asarray(x, dtype=np.float32) - np.asarray(shift, dtype=np.float32)).astype(np.float32)
        sq = (xc * xc).astype(np.float32)
        ok = np.isfinite(sq)
    xc, sq = np.where(ok, xc, np.float32(0)), np.where(ok, sq, np.float32(0))
    return np.concatenate([xc, sq, np.ones((len(xc), 1), dtype=np.float32)], axis=1).astype(dtype)


def accumulate(x, post, shift, n_ranges=0):
    from abnet3_amd import hmm
    sums = hmm.accumulate(x if isinstance(x, torch.Tensor) else dev(x, np.float32), post if isinstance(post, torch.Tensor) else dev(post, np.float32),
                          shift if isinstance(shift, torch.Tensor) else dev(shift, np.float32), n_ranges)
    torch.cuda.synchronize()
    return host(sums)


# ---- 1. the stats entry against the old entry --------------------------------------------------------------------------
@pytest.mark.parametrize('K,D,rho', GRID)
def test_stats_entry_is_the_old_entry_and_stay_k_is_the_restatement(cases, K, D, rho):
    case = cases(K, D)
    got, old = run_stats(case, rho), run_plain(case, rho)
    for k in old:
        assert torch.equal(got[k], old[k]), k
    sk, stays, ng = host(got['stay_k']), host(got['stays']), host(got['n_good'])
    assert list(ng) == [0, 1, 1, 126, 127, 128, 172]
    r = case.scores()
    S = case.per_utterance(r['eps'] + r['delta'])
    bar = ng * np.expm1(2.0 * S)
    ref = reference_stay_k(case, rho)
    e = np.abs(sk - ref)
    e_sum = np.abs(sk.sum(axis=1) - stays)
    live = bar > 0
    print('K%d D%d rho%g: stay_k reaches %.3g of the bar, sum_k stay_k - stays %.3g of it' % (
        K, D, rho, (e[live] / bar[live, None]).max(), (e_sum[live] / bar[live]).max()))
    assert np.isfinite(sk).all() and (sk >= 0).all()
    assert (e <= bar[:, None]).all(), (e / np.maximum(bar[:, None], 1e-300)).max()
    assert (e_sum <= bar).all()
    # zero rows and entries: fewer than two good frames, a component of weight 0, rho = 0, the filtered mode
    assert not sk[:3].any() and not sk[:, 1].any()
    if rho == 0.0:
        assert not sk.any()
    else:
        assert (sk[3:].sum(axis=1) > 0).all()
    filt, old_f = run_stats(case, rho, 'filter'), run_plain(case, rho, 'filter')
    for k in old_f:
        assert torch.equal(filt[k], old_f[k]), k
    assert not host(filt['stay_k']).any()


def test_a_refused_utterance_gets_a_nan_row(cases):
    from abnet3_amd import _lib
    lib = _lib.load()
    case = cases(130, 5)
    d, T, K, D = case.d, T_ROWS, 130, 5
    off = np.array([8, -1, T - 3, 135], dtype=np.int64)
    lens = np.array([127, 4, 4, 128], dtype=np.int32)                # fine, off < 0, past the end, fine
    post = torch.full((T, K), 7.0, dtype=torch.float32, device='cuda')
    ll, st = (torch.zeros(4, dtype=torch.float64, device='cuda') for _ in range(2))
    ng = torch.zeros(4, dtype=torch.int32, device='cuda')
    sk = torch.full((4, K), 5.0, dtype=torch.float64, device='cuda')
    need = lib.abn_hmm_ws_bytes(4, 128, K, D)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    p = _lib.ptr
    rc = lib.abn_hmm_forward_backward_stats(p(d['table']), T, D, p(off_d), p(len_d), 4, p(d['shift']), p(d['A']), p(d['B']), p(d['c0']),
                                            p(d['w']), K, 0.9, 0, p(post), p(ll), p(st), p(ng), p(sk), p(ws), need, _lib.stream())
    assert rc == 0
    torch.cuda.synchronize()
    sk = host(sk)
    assert list(host(ng)) == [126, -1, -1, 127]
    assert np.isnan(sk[1]).all() and np.isnan(sk[2]).all() and np.isfinite(sk[[0, 3]]).all()
    whole = host(run_stats(case, 0.9)['stay_k'])
    assert np.array_equal(sk[0], whole[3]) and np.array_equal(sk[3], whole[4])
    got = host(post)
    assert (got[:8] == 7.0).all() and (got[263:] == 7.0).all()           # rows of no accepted utterance keep what they held


# ---- 2. accumulate on exact arithmetic ---------------------------------------------------------------------------------
@pytest.mark.parametrize('T', [1, 127, 129, 1000])
def test_accumulate_is_exact_on_exact_arithmetic(T):
    """post in {0, 1/4, 1/2, 1}, integer x in [-8, 8], an integer shift in [-3, 3]: every product is a multiple of 1/4 below
    121 and every partial sum of at most 1000 of them is below 2^17, so every fp32 sum is exact in any order."""
    rng = np.random.default_rng(T)
    for K in (1, 130, 300):
        post = rng.choice(np.array([0.0, 0.25, 0.5, 1.0], dtype=np.float32), size=(T, K))
        post_d = dev(post, np.float32)
        for D in (1, 5, 40):
            x = rng.integers(-8, 9, size=(T, D)).astype(np.float32)
            shift = rng.integers(-3, 4, size=D).astype(np.float32)
            want = post.astype(np.float64).T @ augment_elementwise(x, shift)
            x_d, shift_d = dev(x, np.float32), dev(shift, np.float32)
            for n_ranges in (0, 1, 3):
                got = accumulate(x_d, post_d, shift_d, n_ranges)
                assert got.shape == (K, 2 * D + 1)
                assert np.array_equal(got, want), (T, K, D, n_ranges, np.abs(got - want).max())


# ---- 3. accumulate on float data ---------------------------------------------------------------------------------------
@pytest.mark.parametrize('T,K,D,n_ranges', [(1000, 130, 5, 0), (1000, 300, 40, 3), (700, 3, 1, 1), (2000, 513, 13, 2), (129, 130, 100, 0)])
def test_accumulate_on_float_data_with_bad_rows(T, K, D, n_ranges):
    rng = np.random.default_rng(T + K + D)
    x = (rng.normal(size=(T, D)) * 3.0 + 1.0).astype(np.float32)
    shift = x.mean(axis=0).astype(np.float32)
    post = rng.dirichlet(np.full(K, 0.3), size=T).astype(np.float32)
    tail = min(40, T // 4)
    post[T - tail:] = 0.0                                               # rows behind the last utterance: zeros
    bad = np.array(sorted(set([0, T // 2, T - tail - 1, 128 % T])))
    post[bad] = 0.0                                                     # the chain leaves zero rows at BAD frames
    xb = x.copy()
    xb[bad[0], 0], xb[bad[1], D - 1], xb[bad[2], :], xb[T - 1, 0] = np.nan, np.inf, -np.inf, np.nan
    if len(bad) > 3:
        xb[bad[3], D // 2] = 3e19
    aug = augment_elementwise(xb, shift)
    g = post.astype(np.float64)
    want = g.T @ aug
    bar = (frames_per_range(T, K, n_ranges) + 2) * U * (g.T @ np.abs(aug))
    got = accumulate(xb, post, shift, n_ranges)
    e = np.abs(got - want)
    print('T%d K%d D%d n_ranges %d: %.3g of the bar' % (T, K, D, n_ranges, (e / np.maximum(bar, 1e-300)).max()))
    assert np.isfinite(got).all() and (e <= bar).all(), (e / np.maximum(bar, 1e-300)).max()
    # the rows with a non-finite value and the rows behind the last utterance contribute NOTHING: finite values in their
    # place give the same bits
    assert np.array_equal(accumulate(x, post, shift, n_ranges), got)
    xg = x.copy()
    xg[bad], xg[T - tail:] = 1000.0, -77.0
    assert np.array_equal(accumulate(xg, post, shift, n_ranges), got)
    # a non-finite ENTRY under a non-zero responsibility contributes 0 in its own two columns, never 0 x NaN
    post2 = post.copy()
    post2[bad[0]] = 1.0 / K
    want2 = post2.astype(np.float64).T @ aug
    got2 = accumulate(xb, post2, shift, n_ranges)
    bar2 = (frames_per_range(T, K, n_ranges) + 2) * U * (post2.astype(np.float64).T @ np.abs(aug))
    assert np.isfinite(got2).all() and (np.abs(got2 - want2) <= bar2).all()
    assert np.array_equal(accumulate(xb, post, shift, n_ranges), got)    # two calls, the same bits


# ---- 4. cross-checks ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,D', [(130, 5), (300, 40)])
def test_on_the_mixtures_own_posteriors_the_sums_are_abn_gmm_mstep_s(cases, K, D):
    from abnet3_amd import gmm
    case = cases(K, D)
    d = case.d
    w = case.w32.astype(np.float64)
    w = np.where(w > 0, w, 1e-3)                                        # (the mixture wants positive weights)
    m, v = (np.random.default_rng(K).normal(size=(K, D)), np.full((K, D), 1.5))
    st = gmm.EMState(w / w.sum(), m, v, np.ones(D), 'cuda')
    _, g = gmm.posteriors(d['table'], d['shift'], st.A, st.B, st.c)
    ours = accumulate(d['table'], g, d['shift'], 0)
    gmm.em_iteration(d['table'], d['shift'], st, n_ranges=0)
    torch.cuda.synchronize()
    theirs = host(st.sums)
    gh = host(g).astype(np.float64)
    aug = augment_elementwise(case.x, host(d['shift']))
    bar = 2.0 * (frames_per_range(T_ROWS, K, 0) + 2) * U * (gh.T @ np.abs(aug))
    e = np.abs(ours - theirs)
    print('K%d D%d: abn_hmm_accumulate on abn_gmm_posteriors\' table against abn_gmm_mstep\'s sums: %s, %.3g of twice the bar'
          % (K, D, 'EQUAL' if np.array_equal(ours, theirs) else 'not equal', (e / np.maximum(bar, 1e-300)).max()))
    assert (e <= bar).all()


@pytest.mark.parametrize('K,D,rho', GRID[:4])
def test_sums_of_the_kernels_gamma_against_the_float64_restatement(cases, K, D, rho):
    case = cases(K, D)
    got = run_stats(case, rho)
    sums = accumulate(case.d['table'], got['post'], case.d['shift'], 0)
    r = case.scores()
    ref64 = case.reference(rho, True)[0]
    aug = gmm_np.augment(case.xc, case.bad, np.float64)
    want = ref64['post'].T @ aug
    S_rows = np.zeros(T_ROWS)
    S = case.per_utterance(r['eps'] + r['delta'])
    for o, n, s in zip(case.off, case.lens, S):
        S_rows[o:o + n] = s
    inside = np.zeros(T_ROWS, dtype=bool)
    for o, n in zip(case.off, case.lens):
        inside[o:o + n] = True
    allowed_g = np.where((inside & ~case.bad)[:, None], ref64['post'] * np.expm1(2.0 * S_rows)[:, None] + FLOOR, 0.0)
    g = host(got['post']).astype(np.float64)
    bar = (frames_per_range(T_ROWS, K, 0) + 2) * U * (g.T @ np.abs(aug)) + allowed_g.T @ np.abs(aug)
    e = np.abs(sums - want)
    print('K%d D%d rho%g: sums against the float64 restatement reach %.3g of the bar' % (K, D, rho, (e / np.maximum(bar, 1e-300)).max()))
    assert (e <= bar).all(), (e / np.maximum(bar, 1e-300)).max()
    assert not sums[1].any()                                             # the component of weight 0


# ---- 5. reproducibility ------------------------------------------------------------------------------------------------
def test_two_calls_and_every_utterance_alone_give_the_same_bits(cases):
    case = cases(300, 40)
    a, b = run_stats(case, 0.9), run_stats(case, 0.9)
    for k in a:
        assert torch.equal(a[k], b[k]) or k == 'stays' and np.array_equal(host(a[k]), host(b[k])), k
    s1 = accumulate(case.d['table'], a['post'], case.d['shift'], 0)
    assert np.array_equal(s1, accumulate(case.d['table'], b['post'], case.d['shift'], 0))
    whole = host(a['stay_k'])
    for u, (o, n) in enumerate(zip(case.off, case.lens)):
        if n == 0:
            continue
        one = run_stats(case, 0.9, off=[0], lens=[n], table=dev(case.x[o:o + n], np.float32))
        assert np.array_equal(host(one['stay_k'])[0], whole[u]), u
        assert host(one['stays'])[0] == host(a['stays'])[u]


def test_more_utterances_than_workgroups():
    """300 utterances of 3 frames: the persistent loop; the rows in any order, and a few utterances alone."""
    rng = np.random.default_rng(19)
    lens = np.full(300, 3, dtype=np.int64)
    x, shift, w, m, v = make_model(900, 130, 5, seed=19)
    case = Case(x, shift, w, m, v, lens)
    got = run_stats(case, 0.9)
    sk = host(got['stay_k'])
    perm = rng.permutation(300)
    other = run_stats(case, 0.9, off=case.off[perm], lens=case.lens[perm])
    assert torch.equal(other['post'], got['post']) and np.array_equal(host(other['stay_k']), sk[perm])
    for u in (0, 255, 256, 299):
        o = int(case.off[u])
        one = run_stats(case, 0.9, off=[0], lens=[3], table=dev(case.x[o:o + 3], np.float32))
        assert np.array_equal(host(one['stay_k'])[0], sk[u]), u
    ref = reference_stay_k(case, 0.9)
    r = case.scores()
    bar = 3 * np.expm1(2.0 * case.per_utterance(r['eps'] + r['delta']))
    assert (np.abs(sk - ref) <= bar[:, None]).all()


# ---- 6. fit ------------------------------------------------------------------------------------------------------------
def planted_model(seed):
    from abnet3_amd.gmm import GmmPosteriorgram
    x, lens, shift, gv, w, m, v = hmm_bw_np.perturbed_start(seed)
    g = GmmPosteriorgram(4)
    g.weights_, g.means_, g.variances_ = w.copy(), m + shift.astype(np.float64), v.copy()
    g.shift_, g.gv_ = shift, gv
    feats = {'u%03d' % i: x[o:o + n] for i, (o, n) in enumerate(zip(np.cumsum(lens) - lens, lens))}
    return g, x, lens, feats, (shift, gv, w, m, v)


def loglik_bar(x, shift, w, m, v, lens):
    """test_fit_stay_recovers_the_planted_stay's bar on the mean log-likelihood per good frame under one model."""
    case = Case(x, shift, w, m, v, lens)
    r = case.scores()
    mx = np.where(case.w32 > 0, r['s64'], -np.inf).max(axis=1)
    return float((r['eps'] + r['delta'] + 2.0 * U * np.abs(mx)).sum() / len(x))


def scaled(a, ref):
    return float(np.abs(np.asarray(a, dtype=np.float64) - ref).max() / np.abs(ref).max())


@pytest.mark.parametrize('seed', [0, 1])
def test_fit_on_a_planted_corpus(seed):
    """The yardstick measured on the CPU (the float32 restatement against the float64 one after the same 8 iterations, the
    largest difference over the array's largest magnitude): seed 0: stay 1.33e-7, weights 3.81e-6, means 6.97e-7,
    variances 1.80e-5; seed 1: stay 6.63e-8, weights 1.03e-5, means 1.45e-6, variances 2.85e-5.  So every array is held to
    4 x yardstick, all above 2^-22 = 2.4e-7: 5.3e-7 / 2.65e-7 (stay), 1.5e-5 / 4.1e-5 (weights), 2.8e-6 / 5.8e-6 (means),
    7.2e-5 / 1.1e-4 (variances).  The test measures the yardstick again and prints the kernel's figure beside it."""
    from abnet3_amd.hmm import StickyHmmPosteriorgram
    g, x, lens, feats, (shift, gv, w, m, v) = planted_model(seed)
    before = (g.weights_.copy(), g.means_.copy(), g.variances_.copy())
    h = StickyHmmPosteriorgram(g, 0.5).fit(feats, n_iter=8, tol=-np.inf)
    assert h.gmm is not g and all(np.array_equal(a, b) for a, b in zip((g.weights_, g.means_, g.variances_), before))
    assert len(h.log_likelihoods) == 8 and h.n_bad_ == 0 and h.n_retired_ == 0 and h.n_starved_ == 0
    xc, bad = gmm_np.centre(x, shift)
    off = np.cumsum(lens) - lens
    ref = hmm_bw_np.em(xc, bad, off, lens, w, m, v, 0.5, gv, n_iter=8, var_floor=g.var_floor, min_count=g.min_count)
    r32 = hmm_bw_np.em(xc, bad, off, lens, w, m, v, 0.5, gv, n_iter=8, var_floor=g.var_floor, min_count=g.min_count, dtype=np.float32)
    print('seed %d: log-likelihoods %s' % (seed, ' '.join('%.5f' % l for l in h.log_likelihoods)))
    # non-decreasing within the two likelihoods' bars (the models of the float64 EM: one bar per iteration)
    models = [(w, m, v)]
    wi, mi, vi, ri = w, m, v, 0.5
    for _ in range(7):
        e = hmm_bw_np.e_step(xc, bad, off, lens, wi, mi, vi, ri)
        wi, mi, vi, ri, _ = hmm_bw_np.m_step(e['sums'], e['stay_k'].sum(axis=0), int(np.maximum(e['n_good'] - 1, 0).sum()), wi, mi, vi,
                                             ri, gv, g.var_floor, g.min_count)
        models.append((wi, mi, vi))
    bars = np.array([loglik_bar(x, shift, *mod, lens) for mod in models])
    d = np.diff(h.log_likelihoods)
    assert (d >= -(bars[1:] + bars[:-1])).all(), (d, bars)
    got = dict(rho=h.stay_, w=h.gmm.weights_, m=h.gmm.means_ - shift.astype(np.float64), v=h.gmm.variances_)
    for k in ('rho', 'w', 'm', 'v'):
        yard = scaled(r32[k], np.asarray(ref[k], dtype=np.float64))
        tol = max(FLOOR, 4.0 * yard)
        err = scaled(got[k], np.asarray(ref[k], dtype=np.float64))
        print('seed %d %s: kernel %.3g, float32 restatement %.3g, allowed %.3g' % (seed, k, err, yard, tol))
        assert err <= tol, (k, err, tol)


def test_fit_of_the_stay_alone_is_fit_stay_and_files_and_corpus_forms(tmp_path):
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.hmm import StickyHmmPosteriorgram
    g, x, lens, feats, _ = planted_model(0)
    a = StickyHmmPosteriorgram(g, 0.5).fit_stay(feats, n_iter=4, tol=-np.inf)
    b = StickyHmmPosteriorgram(g, 0.5).fit(feats, n_iter=4, tol=-np.inf, params='s')
    assert b.stay_ == a.stay_ and b.log_likelihoods == a.log_likelihoods
    assert np.array_equal(b.gmm.means_, g.means_) and np.array_equal(b.gmm.weights_, g.weights_)
    # the three corpus forms
    times = {k: np.arange(len(f), dtype=np.float64) * 0.01 for k, f in feats.items()}
    corpus = DeviceCorpus(feats, times)
    h = StickyHmmPosteriorgram(g, 0.5).fit(feats, n_iter=3, tol=-np.inf)
    hc = StickyHmmPosteriorgram(g, 0.5).fit(corpus, n_iter=3, tol=-np.inf)
    assert hc.stay_ == h.stay_ and hc.log_likelihoods == h.log_likelihoods
    for k in ('weights_', 'means_', 'variances_'):
        assert np.array_equal(getattr(hc.gmm, k), getattr(h.gmm, k)), k
    one = StickyHmmPosteriorgram(g, 0.5).fit(corpus.table, n_iter=3, tol=-np.inf)       # ONE utterance of 3000 frames
    assert len(one.log_likelihoods) == 3 and np.isfinite(one.log_likelihoods).all() and one.log_likelihoods[-1] > one.log_likelihoods[0]
    assert abs(one.gmm.weights_.sum() - 1.0) <= 1e-12
    # the stopping rule: a huge tolerance stops after the second likelihood, the first update applied
    two = StickyHmmPosteriorgram(g, 0.5).fit(feats, n_iter=8, tol=1e9)
    assert two.log_likelihoods == h.log_likelihoods[:2]
    # save -> load -> transform: the same bits
    path = str(tmp_path / 'bw.npz')
    h.save(path)
    h2 = StickyHmmPosteriorgram.load(path)
    assert h2.stay_ == h.stay_ and np.array_equal(h2.gmm.means_, h.gmm.means_)
    assert torch.equal(h2.transform(corpus).table, h.transform(corpus).table)


# ---- 7. host refusals reached through the device path -------------------------------------------------------------------
def test_refusals_before_any_launch():
    from abnet3_amd import hmm
    g, x, lens, feats, _ = planted_model(0)
    h = hmm.StickyHmmPosteriorgram(g, 0.5)
    with pytest.raises(ValueError, match='D = 5'):
        h.fit(torch.zeros(50, 5, device='cuda'))
    with pytest.raises(ValueError, match='abn_hmm_max_len'):
        h.fit(torch.zeros(hmm.max_len() + 1, 3, device='cuda'))
    with pytest.raises(ValueError, match='params'):
        h.fit(feats, params='mvz')
    with pytest.raises(ValueError, match='abn_hmm_max_k'):
        hmm.accumulate(torch.zeros(4, 3, device='cuda'), torch.zeros(4, hmm.max_k() + 1, device='cuda'), torch.zeros(3, device='cuda'))
    assert h.gmm is g and h.log_likelihoods == [] and h.stay_ == 0.5
