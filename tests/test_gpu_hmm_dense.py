"""abny_hmm_dense_forward_backward and TransitionHmmPosteriorgram on the MI355X against tests/hmm_dense_np.py.

The error bars (all derived, none tuned).  The emission scores carry tests/test_gpu_hmm.py's score bar eps_t (the float32
numpy scores' own scaled maximum error against float64 as the yardstick, bar = max(2^-22, 4 x yardstick), times the
frame's largest score scale).  The chain adds delta = (2 K + 21) 2^-24 per good frame, counted from csrc/hmm_dense.hip's
operations.  Forward, K + 17: the subtraction and the exp (2); the dot product sum_j ahat[j] trans[j][k], K fused
multiply-adds whose partial sums are combined slice by slice -- however a sum of K non-negative terms is grouped, no
term passes more than K roundings, and adding an exact zero (the padding past K) rounds nothing -- (K); the product
with bt (1); the sum c_t, four DPP steps, three row sums and three wave sums (12); the reciprocal and its product (2).
Backward, K + 4: the two products and the reciprocal of e = bt bhat / c_t (3), the dot product sum_k trans[j][k] e[k] (K),
the product gamma = ahat bhat (1).  Perturbing every factor of every path by at most e^(+-(eps_t + delta)) moves a
ratio of path sums by at most e^(+-2 S), S = the sum of eps_t + delta over the utterance's good frames.  So
    gamma, ahat: |d| <= g64 expm1(2 S) + 2^-22;   |sum_k gamma - 1| <= expm1(2 S) + 2^-22;
    loglik: |d| <= S + 2 x 2^-24 sum_t |m_t|;
    xi[j][k], first[k]: |d| <= ref (expm1(2 S_max) + 129 x 2^-24) + 2^-22 x (the transitions / first frames that feed the cell):
      each term is a ratio of path sums; a thread adds at most 128 of them in fp32 (one fused multiply-add each: 129
      roundings with the product) before they go into float64.
Tight checks free of the score term: the sticky matrix against abn_hmm_forward_backward_stats (the slabs carry the same
bits; only the two chains' delta enter, (2 K + 21) + (K + 16) per frame); all rows of trans equal to w against
abn_gmm_posteriors; K = 1.  Each grid case prints the kernel's error over the float32 restatement's own (-s shows it).

Largest kernel / float32-restatement error ratios seen on the MI355X over all grid cases: see RECORDED below."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import hmm_dense_np as dn  # noqa: E402
from test_gpu_hmm import Case, make_model, dev, host, U, FLOOR, LENS  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT2_SYMBOLS: the entry the dirty-memory test below reaches, and the two host queries
DIRTY_CASES = ('abny_hmm_dense_forward_backward',)
QUERIES = ('abny_hmm_dense_max_k', 'abny_hmm_dense_ws_bytes')

MAX_K = 128                                                  # (asserted against abny_hmm_dense_max_k below)
KS = (1, 2, 5, 64, 65, 127, MAX_K)
DS = (1, 13, 40)
RATIOS = {'gamma': 0.0, 'ahat': 0.0, 'loglik': 0.0, 'xi': 0.0, 'first': 0.0}
# RECORDED: the largest ratios a full run of this file printed on the MI355X (kernel error / float32 restatement's error)
RECORDED = ('gamma 2.28 (K = 5, D = 13: kernel 2.43e-6 against 1.07e-6, 0.024 of its bar), ahat 1.40, loglik 2.94 (K = 1, D = 40: '
            '6.6e-5 against 2.3e-5 nats, 0.024 of its bar), xi 2.49 (K = 5, D = 13: 2.2e-5 against 9.0e-6, 5.6e-5 of its bar), first 3.05 '
            '(K = 5, D = 13: 2.2e-6 against 7.4e-7, 1.1e-4 of its bar); the bars themselves were reached to 0.070 (gamma, the 300 short utterances) and 0.084 '
            '(loglik, K = 2, D = 13) at most; the sticky kernel 0.007 (post), 0.006 (loglik), 3e-4 (stay_k); abn_gmm_posteriors 0.46 (gamma, K = 5)')


def delta_dense(K):
    return (2 * K + 21) * U


def random_transitions(K, seed, sticky=0.0):
    """init [K], trans [K, K] float32: Dirichlet rows, mixed with the identity by `sticky`."""
    rng = np.random.default_rng(seed)
    init = rng.dirichlet(np.full(K, 2.0))
    trans = (1.0 - sticky) * rng.dirichlet(np.full(K, 2.0), size=K) + sticky * np.eye(K)
    return init.astype(np.float32), np.ascontiguousarray(trans.astype(np.float32))


class DenseCase(Case):
    """test_gpu_hmm.Case (the device tables of a model, its float64 / float32 scores and their bar) with init and trans."""

    def __init__(self, x, shift, w, m, v, lens, init, trans):
        Case.__init__(self, x, shift, w, m, v, lens)
        self.init, self.trans = init, trans
        self.d['init'], self.d['trans'] = dev(init, np.float32), dev(trans, np.float32)

    def run(self, mode='smooth', off=None, lens=None, table=None, out=None, want_stats=True, init=None, trans=None):
        from abnet3_amd import hmm
        d = self.d
        r = hmm.dense_forward_backward(d['table'] if table is None else table, self.off if off is None else off,
                                       self.lens if lens is None else lens, d['shift'], d['A'], d['B'], d['c0'],
                                       d['init'] if init is None else init, d['trans'] if trans is None else trans, mode, out=out,
                                       want_stats=want_stats)
        torch.cuda.synchronize()
        got = dict(post=host(r[0]), loglik=host(r[1]), n_good=host(r[2]))
        if want_stats:
            got['stats'] = host(r[3])
        return got

    def scores(self):
        r = Case.scores(self)
        r['delta'] = np.where(~self.bad, delta_dense(self.K), 0.0)
        return r

    def reference(self, smooth=True):
        key = ('dense', smooth)
        if key not in self._ref:
            r = self.scores()
            self._ref[key] = (dn.corpus(r['s64'], self.bad, self.off, self.lens, self.init, self.trans, np.float64, smooth),
                              dn.corpus(r['s32'], self.bad, self.off, self.lens, self.init, self.trans, np.float32, smooth))
        return self._ref[key]


def stats_bar(ref_stats, n_good, S_max):
    """The docstring's bar on stats [K + 1, K] from the float64 reference, the utterances' good-frame counts and S_max."""
    K = ref_stats.shape[1]
    feed = np.concatenate([np.full((K, K), np.maximum(n_good - 1, 0).sum()), np.full((1, K), (n_good > 0).sum())]).astype(np.float64)
    return ref_stats * (np.expm1(2.0 * S_max) + 129 * U) + FLOOR * feed


def check_against_reference(case, got, smooth, tag):
    """The module docstring's bars on the posteriors, the row sums, loglik, n_good and the statistics; fills RATIOS."""
    r = case.scores()
    ref64, ref32 = case.reference(smooth)
    good = ~case.bad
    S = case.per_utterance(r['eps'] + r['delta'])
    S_rows = case.rows(S)
    assert np.array_equal(got['n_good'], ref64['n_good'])
    assert np.isfinite(got['post']).all() and not got['post'][case.bad].any()
    g64 = ref64['post']
    allowed = g64 * np.expm1(2.0 * S_rows)[:, None] + FLOOR
    e_g = np.abs(got['post'].astype(np.float64) - g64)
    e_32 = np.abs(ref32['post'].astype(np.float64) - g64)
    name = 'gamma' if smooth else 'ahat'
    ratio = e_g.max() / max(e_32.max(), FLOOR / 4)
    RATIOS[name] = max(RATIOS[name], ratio)
    e_ll = np.abs(got['loglik'] - ref64['loglik'])
    y_ll = np.abs(ref32['loglik'] - ref64['loglik'])
    bar_ll = S + 2.0 * U * case.per_utterance(np.abs(ref64['m']))
    ratio_ll = e_ll.max() / max(y_ll.max(), FLOOR / 4)
    RATIOS['loglik'] = max(RATIOS['loglik'], ratio_ll)
    print('%s: %s kernel %.3g restatement32 %.3g (ratio %.2f), of the bar %.3g; loglik kernel %.3g restatement32 %.3g (ratio %.2f), '
          'of the bar %.3g' % (tag, name, e_g.max(), e_32.max(), ratio, (e_g / allowed).max(), e_ll.max(), y_ll.max(), ratio_ll,
                               (e_ll / np.maximum(bar_ll, 1e-300)).max()))
    assert (e_g <= allowed).all(), (tag, (e_g / allowed).max())
    sums = got['post'].astype(np.float64).sum(axis=1)
    assert (np.abs(sums[good] - 1.0) <= np.expm1(2.0 * S_rows[good]) + FLOOR).all(), (tag, np.abs(sums[good] - 1.0).max())
    assert (e_ll <= bar_ll).all(), (tag, (e_ll / np.maximum(bar_ll, 1e-300)).max())
    if 'stats' not in got:
        return
    if not smooth:
        assert not got['stats'].any()
        return
    K = case.K
    ref_st = np.concatenate([ref64['xi'], ref64['first'][None, :]])
    st32 = np.concatenate([ref32['xi'], ref32['first'][None, :]])
    bar = stats_bar(ref_st, ref64['n_good'], S.max() if len(S) else 0.0)
    e_st, y_st = np.abs(got['stats'] - ref_st), np.abs(st32 - ref_st)
    for nm, sl in (('xi', slice(0, K)), ('first', slice(K, K + 1))):
        ratio_st = e_st[sl].max() / max(y_st[sl].max(), FLOOR / 4)
        RATIOS[nm] = max(RATIOS[nm], ratio_st)
        print('%s: %s kernel %.3g restatement32 %.3g (ratio %.2f), of the bar %.3g' % (tag, nm, e_st[sl].max(), y_st[sl].max(), ratio_st,
                                                                                 (e_st[sl] / bar[sl]).max()))
    assert (got['stats'] >= 0).all() and (e_st <= bar).all(), (tag, (e_st / bar).max())
    assert abs(got['stats'][:K].sum() - np.maximum(ref64['n_good'] - 1, 0).sum()) <= bar[:K].sum()


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(K, D, seed=0, sticky=0.5, **kw):
        key = (K, D, seed, sticky) + tuple(sorted(kw.items()))
        if key not in cache:
            x, shift, w, m, v = make_model(int(sum(LENS)), K, D, seed=1000 * K + D + seed, **kw)
            init, trans = random_transitions(K, 7 * K + D + seed, sticky)
            cache[key] = DenseCase(x, shift, w, m, v, LENS, init, trans)
        return cache[key]
    return get


def test_the_limit_is_the_one_this_file_was_written_for():
    from abnet3_amd import hmm
    assert hmm.dense_max_k() == MAX_K >= 128


@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_smoothed_and_filtered_on_the_shape_grid(cases, K, D):
    case = cases(K, D)
    tag = 'K%d D%d' % (K, D)
    check_against_reference(case, case.run('smooth'), True, tag)
    check_against_reference(case, case.run('filter'), False, tag + ' filter')
    print('largest kernel / float32-restatement ratios so far:', RATIOS)


@pytest.mark.parametrize('K,D,rho', [(2, 1, 0.5), (5, 13, 0.9), (64, 40, 0.0), (65, 13, 0.999), (MAX_K, 40, 0.9)])
def test_sticky_matrix_against_the_sticky_kernel(cases, K, D, rho):
    """init = w32 and the sticky matrix against abn_hmm_forward_backward_stats on the same inputs.  Both chains start from
    the same bt bits, so only their own roundings enter: S = n_good ((2 K + 21) + (K + 16)) 2^-24 per utterance.  post within
    g expm1(2 S) + 2^-22, loglik within S, and stay_k[k] = xi[k][k] stay / (stay + (1 - stay) w[k]) within the statistics' bar."""
    from abnet3_amd import hmm
    case = cases(K, D)
    d = case.d
    init, trans = hmm.sticky_transitions(case.w32, rho)
    assert np.array_equal(init, dn.sticky_matrix(case.w32, rho)[0]) and np.array_equal(trans, dn.sticky_matrix(case.w32, rho)[1])
    got = case.run(init=dev(init, np.float32), trans=dev(trans, np.float32))
    post, ll, st, ng, sk = hmm.forward_backward(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], d['w'], rho,
                                                'smooth', want_stay_k=True)
    torch.cuda.synchronize()
    post, ll, ng, sk = host(post).astype(np.float64), host(ll), host(ng), host(sk).sum(axis=0)
    assert np.array_equal(got['n_good'], ng)
    S = ng * (delta_dense(K) + (K + 16) * U)
    allowed = post * np.expm1(2.0 * case.rows(S))[:, None] + FLOOR
    e_g = np.abs(got['post'] - post)
    e_ll = np.abs(got['loglik'] - ll)
    r32, omr = float(np.float32(rho)), float(np.float32(1.0) - np.float32(rho))
    stay_k = np.diag(got['stats'][:K]) * r32 / (r32 + omr * case.w32.astype(np.float64))
    bar_sk = sk * (np.expm1(2.0 * S.max()) + 129 * U) + FLOOR * np.maximum(ng - 1, 0).sum()
    print('K%d D%d rho%g: post %.3g of its bar, loglik %.3g of its bar, stay_k %.3g of its bar'
          % (K, D, rho, (e_g / allowed).max(), (e_ll / np.maximum(S, 1e-300)).max(), (np.abs(stay_k - sk) / bar_sk).max()))
    assert (e_g <= allowed).all(), (e_g / allowed).max()
    assert (e_ll <= S).all(), (e_ll / np.maximum(S, 1e-300)).max()
    assert (np.abs(stay_k - sk) <= bar_sk).all(), (np.abs(stay_k - sk) / bar_sk).max()


@pytest.mark.parametrize('K,D', [(1, 1), (5, 13), (64, 40), (127, 13), (MAX_K, 40)])
def test_equal_rows_are_abn_gmm_posteriors(cases, K, D):
    """All rows of trans equal to w and init = w, with equal weights, against abn_gmm_posteriors on the very table the
    kernel reads (c0; a constant log w added to every component moves no posterior).  Both start from the same score
    bits.  gamma = ahat bhat: ahat carries the forward count twice (the numerator and c_t), 2 (K + 17), bhat the backward
    count K + 4, the mixture's route K + 4 (exp, sum, division): g (4 K + 42) 2^-24 + 2^-22.  loglik: c_t carries the dot
    product (K), the sum of the previous ahat (14), the exp (2), the product (1) and its own sum (12); the mixture's lse its
    sum and rounding: sum_t ((2 K + 33) 2^-24 + 2^-23 |lse_t|) against sum_t (lse_t + log w)."""
    from abnet3_amd import gmm
    case = cases(K, D, uniform=True)
    w32 = np.float32(1.0 / K)
    assert (case.w32 == w32).all()
    init, trans = np.full(K, w32, dtype=np.float32), np.full((K, K), w32, dtype=np.float32)
    got = case.run(init=dev(init, np.float32), trans=dev(trans, np.float32))
    d = case.d
    lse, g = gmm.posteriors(d['table'], d['shift'], d['A'], d['B'], d['c0'])
    lse, g = host(lse).astype(np.float64) + np.log(np.float64(w32)), host(g).astype(np.float64)
    e_g = np.abs(got['post'] - g)
    allowed = g * (4 * K + 42) * U + FLOOR
    bar_ll = case.per_utterance((2 * K + 33) * U + 2.0 ** -23 * np.abs(lse))
    e_ll = np.abs(got['loglik'] - case.per_utterance(lse))
    print('K%d D%d: gamma %.3g of its bar, loglik %.3g of its bar' % (K, D, (e_g / allowed).max(), (e_ll / bar_ll).max()))
    assert (e_g <= allowed).all(), (e_g / allowed).max()
    assert (e_ll <= bar_ll).all(), (e_ll / bar_ll).max()


def test_one_component_gives_exactly_one(cases):
    """K = 1: bt = 1, init = trans = 1, and every product and sum of the chain is exact."""
    case = cases(1, 13)
    one = dev(np.ones(1), np.float32)
    for mode in ('smooth', 'filter'):
        got = case.run(mode, init=one, trans=one.reshape(1, 1))
        assert (got['post'] == 1.0).all()
    assert np.array_equal(got['n_good'], case.lens)
    got = case.run('smooth', init=one, trans=one.reshape(1, 1))
    assert got['stats'][0, 0] == float(np.maximum(case.lens - 1, 0).sum()) and got['stats'][1, 0] == float(len(case.lens))


def test_two_calls_and_every_utterance_alone_give_the_same_bits(cases):
    bits = dirty_memory.bits
    case = cases(65, 40)
    a, b = case.run(), case.run()
    for k in a:
        assert np.array_equal(bits(a[k]), bits(b[k])), k
    plain = case.run(want_stats=False)                            # without the statistics: the same bits elsewhere
    for k in plain:
        assert np.array_equal(bits(plain[k]), bits(a[k])), k
    f = case.run('filter')
    total = np.zeros_like(a['stats'])
    for u, (o, n) in enumerate(zip(case.off, case.lens)):
        for mode, whole in (('smooth', a), ('filter', f)):
            one = case.run(mode, off=[0], lens=[n], table=dev(case.x[o:o + n], np.float32))
            assert np.array_equal(one['post'], whole['post'][o:o + n]), (u, mode)
            assert one['loglik'][0] == whole['loglik'][u] and one['n_good'][0] == n
            if mode == 'smooth':
                total += one['stats']
    # one utterance per workgroup: the corpus' statistics are the float64 sum of the utterances' (trans is applied to the
    # sum there and to every term here: float64 roundings apart)
    assert np.abs(total - a['stats']).max() <= 16 * 2.0 ** -52 * a['stats'].max()


def test_more_utterances_than_workgroups():
    """300 utterances of 1 .. 3 frames at K = 5: the persistent loop.  Every utterance as in the restatement, the posteriors
    in any order, and the statistics the float64 sum of the per-utterance statistics: within the bar of the restatement's,
    and within float64 rounding (300 additions in another order) of the kernel's own, one call per utterance."""
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 4, size=300)
    K, D = 5, 13
    x, shift, w, m, v = make_model(int(lens.sum()), K, D, seed=9)
    init, trans = random_transitions(K, 9, 0.5)
    case = DenseCase(x, shift, w, m, v, lens, init, trans)
    got = case.run()
    check_against_reference(case, got, True, '300 utterances')
    perm = rng.permutation(300)
    other = case.run(off=case.off[perm], lens=case.lens[perm])
    assert np.array_equal(other['post'], got['post']) and np.array_equal(other['loglik'], got['loglik'][perm])
    ref64 = case.reference(True)[0]
    S = case.per_utterance(case.scores()['eps'] + case.scores()['delta'])
    ref_st = np.concatenate([ref64['xi_utt'].sum(axis=0), ref64['first_utt'].sum(axis=0)[None, :]])
    assert (np.abs(other['stats'] - ref_st) <= stats_bar(ref_st, ref64['n_good'], S.max())).all()
    total = np.zeros((K + 1, K))
    for o, n in zip(case.off, case.lens):
        total += case.run(off=[o], lens=[n])['stats']
    assert np.abs(got['stats'] - total).max() <= 300 * 2.0 ** -52 * total.max()
    assert np.abs(other['stats'] - total).max() <= 300 * 2.0 ** -52 * total.max()


def test_bad_rows_are_zero_counted_and_passed_over():
    K, D = 65, 39
    x, shift, w, m, v = make_model(int(sum(LENS)), K, D, seed=4)
    rows = [0, 3, 130, 257, 258, 400, 686]               # (utterances start at 0, 1, 3, 130, 258, 387)
    xb = x.copy()
    xb[0, 3], xb[3, 0], xb[130, 38], xb[257, :], xb[258, 5], xb[400, 7], xb[686, 1] = np.nan, np.inf, -np.inf, np.nan, 3e19, np.inf, np.nan
    init, trans = random_transitions(K, 4, 0.5)
    case = DenseCase(xb, shift, w, m, v, LENS, init, trans)
    assert list(np.flatnonzero(case.bad)) == rows        # 3e19: the overflow of xc^2
    got = case.run()
    check_against_reference(case, got, True, 'bad rows')
    assert not got['post'][rows].any()
    assert list(got['n_good']) == [0, 2, 126, 126, 128, 298]      # an all-BAD utterance, a BAD first frame (3, 130, 258), a BAD last (257, 686)
    assert got['loglik'][0] == 0.0
    assert abs(got['stats'][K].sum() - 5.0) <= 1e-4 and abs(got['stats'][:K].sum() - (1 + 125 + 125 + 127 + 297)) <= 1e-2
    # passed over: the table without the rows gives the other rows' bits (loglik: the blocks of its float64 sum move)
    keep = np.setdiff1d(np.arange(len(x)), rows)
    lens2 = [2, 126, 126, 128, 298]                      # (the first utterance was its BAD frame alone)
    clean = DenseCase(xb[keep], shift, w, m, v, lens2, init, trans).run()
    assert np.array_equal(clean['post'], got['post'][keep])
    assert np.array_equal(clean['n_good'], got['n_good'][1:])
    assert np.abs(clean['loglik'] - got['loglik'][1:]).max() <= 1e-12 * np.abs(got['loglik']).max()
    # (the statistics' fp32 block sums move with the blocks: equal within the 129 roundings of a block sum)
    assert np.abs(clean['stats'] - got['stats']).max() <= 129 * U * got['stats'].max() + FLOOR


# ---- straight at the library ---------------------------------------------------------------------------------------------------
def raw_dense(case, off, lens, mode=0, fill=None, want_stats=True, ws_len=None):
    """(post, loglik, n_good, stats) host arrays of abny_hmm_dense_forward_backward with every output and the workspace from
    torch.empty (fill: `post` is filled first)."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    d, T, K, D, n = case.d, len(case.x), case.K, case.D, len(off)
    post = torch.empty((T, K), dtype=torch.float32, device='cuda')
    if fill is not None:
        post.fill_(fill)
    ll = torch.empty(n, dtype=torch.float64, device='cuda')
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    stats = torch.empty((K + 1, K), dtype=torch.float64, device='cuda') if want_stats else None
    need = lib.abny_hmm_dense_ws_bytes(n, max(1, int(np.max(lens))) if ws_len is None else ws_len, K, D)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    rc = lib.abny_hmm_dense_forward_backward(p(d['table']), T, D, p(off_d), p(len_d), n, p(d['shift']), p(d['A']), p(d['B']), p(d['c0']),
                                             p(d['init']), p(d['trans']), K, mode, p(post), p(ll), p(ng), p(stats), p(ws), need,
                                             _lib.stream())
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(post), host(ll), host(ng), host(stats) if want_stats else None


def test_utterances_outside_the_table_are_left_untouched(cases):
    """A bad off / len marks its utterance and touches nothing; rows outside every utterance keep what they held; the
    statistics hold the one good utterance alone."""
    case = cases(5, 13)
    T = len(case.x)
    off = np.array([0, -1, 10, T - 3, 30], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300], dtype=np.int32)          # fine, off < 0, len < 0, past the end, longer than the workspace holds
    post, ll, ng, stats = raw_dense(case, off, lens, fill=7.0, ws_len=100)
    assert list(ng) == [5, -1, -1, -1, -1] and np.isfinite(ll[0]) and np.isnan(ll[1:]).all()
    assert (post[5:] == 7.0).all() and np.abs(post[:5].sum(axis=1) - 1.0).max() < 1e-5
    alone = case.run(off=[0], lens=[5])
    assert np.array_equal(alone['post'][:5], post[:5]) and alone['loglik'][0] == ll[0]
    assert np.array_equal(dirty_memory.bits(alone['stats']), dirty_memory.bits(stats))


def test_every_next2_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT2_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT2_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS))


@pytest.mark.parametrize('K', [5, 65])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(cases, K):
    """The entry of DIRTY_CASES with post, the per-utterance outputs, the statistics and the workspace from torch.empty under
    the three patterns: the same bits (rows outside every utterance keep the pattern), in both modes, and they are the bits
    of the wrapper's call, whose outputs start from zeros."""
    from abnet3_amd import _lib
    case = cases(K, 40)
    T = len(case.x)
    lens = np.array([1, 2, 127, 128, 129, 290], dtype=np.int64)              # a gap of two rows behind every utterance but the last
    off = np.array([0, 3, 7, 136, 266, 397], dtype=np.int64)
    assert off[-1] + lens[-1] == T and ((off + lens)[:-1] + 2 == off[1:]).all()
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    bits = dirty_memory.bits
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                s, f = raw_dense(case, off, lens, 0), raw_dense(case, off, lens, 1)
            assert int(count) >= 10 and count.nbytes > 2 * T * K * 4          # post, three outputs and the workspace, twice
            word = int.from_bytes(bytes([byte]) * 4, 'little')
            for r in (s, f):
                assert (bits(r[0][~inside]) == word).all() and (~inside).sum() == 10
            outs[byte] = [s[0][inside]] + list(s[1:]) + [f[0][inside]] + list(f[1:])
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert all(np.array_equal(bits(a), bits(b)) for a, b in zip(outs[byte], outs[0x00])), hex(byte)
    # the wrapper's run on the same utterances (zeroed outputs, what the tests above check): the same bits again
    mine = case.run(off=off, lens=lens)
    assert np.array_equal(bits(mine['post'][inside]), bits(outs[0xFF][0])) and np.array_equal(bits(mine['stats']), bits(outs[0xFF][3]))
    assert np.array_equal(bits(mine['loglik']), bits(outs[0xFF][1])) and np.array_equal(mine['n_good'], lens)
    assert not outs[0xFF][7].any() and np.isfinite(outs[0xFF][3]).all()


# ---- end to end --------------------------------------------------------------------------------------------------------
def planted_model(seed=0):
    from abnet3_amd.gmm import GmmPosteriorgram
    x, lens, mu, _ = dn.planted_cycle(seed)
    K, D = mu.shape
    g = GmmPosteriorgram(K)
    g.weights_, g.means_, g.variances_ = np.full(K, 1.0 / K), mu.astype(np.float64), np.ones_like(mu)
    g.shift_, g.gv_ = x.astype(np.float64).mean(axis=0).astype(np.float32), np.ones(D)
    return g, x, lens


def test_fit_on_a_planted_cyclic_model():
    from abnet3_amd.hmm import TransitionHmmPosteriorgram
    g, x, lens = planted_model(0)
    K = g.means_.shape[0]
    feats = {'u%03d' % i: x[o:o + n] for i, (o, n) in enumerate(zip(np.cumsum(lens) - lens, lens))}
    h = TransitionHmmPosteriorgram(g, stay=0.5).fit(feats, n_iter=8, tol=-np.inf, params='ti')
    print('fit: log-likelihoods %s\ntrans\n%s\ninit %s' % (' '.join('%.5f' % v for v in h.log_likelihoods), h.trans_, h.init_))
    assert len(h.log_likelihoods) == 8 and h.n_bad_ == 0 and h.gmm is not g and np.array_equal(h.gmm.means_, g.means_)
    # non-decreasing within the loglik bar (per good frame): the score bar and the chain's delta of every frame
    init0, trans0 = dn.sticky_matrix(g.weights_, 0.5)
    case = DenseCase(x, g.shift_, g.weights_, g.means_ - g.shift_.astype(np.float64), g.variances_, lens, init0, trans0)
    r = case.scores()
    bar = float((r['eps'] + r['delta'] + 2.0 * U * np.abs(r['s64'].max(axis=1))).sum() / len(x))
    assert (np.diff(h.log_likelihoods) >= -2.0 * bar).all(), (np.diff(h.log_likelihoods), bar)
    # (2 bar: each of the two likelihoods of a difference carries the bar)
    assert h.log_likelihoods[-1] > h.log_likelihoods[0] + 100.0 * bar           # and it did rise
    for k in range(K):
        offd = h.trans_[k].copy()
        offd[k] = -1.0
        assert int(np.argmax(offd)) == (k + 1) % K, h.trans_
    assert np.abs(np.diag(h.trans_) - 0.8).max() <= 0.05 and h.trans_.min() >= 2.0 ** -81
    assert np.abs(h.trans_.sum(axis=1) - 1.0).max() <= 1e-12 and abs(h.init_.sum() - 1.0) <= 1e-12
    # the first likelihood is the start's, the fitted model's score is the update of the last one: against the restatement
    ref0 = dn.corpus(r['s64'], case.bad, case.off, case.lens, init0, trans0)
    assert abs(h.log_likelihoods[0] - ref0['loglik'].sum() / len(x)) <= bar
    i32, t32 = h.init_.astype(np.float32), h.trans_.astype(np.float32)
    ref1 = dn.corpus(r['s64'], case.bad, case.off, case.lens, i32, t32, smooth=False)
    assert abs(h.score(feats) - ref1['loglik'].sum() / len(x)) <= bar
    # every parameter at once: the likelihood rises, the mixture moves, the count of starved components is kept
    a = TransitionHmmPosteriorgram(g, stay=0.5).fit(feats, n_iter=3, tol=-np.inf)
    assert len(a.log_likelihoods) == 3 and a.log_likelihoods[-1] > a.log_likelihoods[0] and a.n_starved_ == 0
    assert not np.array_equal(a.gmm.means_, g.means_) and not np.array_equal(a.gmm.variances_, g.variances_)
    assert np.abs(a.gmm.means_ - g.means_).max() < 0.5


def test_transform_of_a_corpus_and_downstream(tmp_path):
    from abnet3_amd import gmm, hmm
    from abnet3_amd.abx import ABXEvaluator, kl_tables
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=60, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    s = hmm.StickyHmmPosteriorgram(g, 0.8)
    h = hmm.TransitionHmmPosteriorgram.from_sticky(s)
    post = h.transform(corpus)
    assert isinstance(post, DeviceCorpus) and post.names == corpus.names and post.dim == 8 and post.total == corpus.total
    for k in corpus.names:
        assert post.length[k] == corpus.length[k] and post.offset[k] == corpus.offset[k]
        assert np.array_equal(post.times[k], corpus.times[k])
    assert torch.equal(h.transform(feats), post.table)                            # the dict form: row for row
    assert int(kl_tables(post.table).bad.sum().item()) == 0
    assert abs(float(post.table.sum(dim=1).mean().item()) - 1.0) < 1e-5
    assert float((post.table - s.transform(corpus).table).abs().max().item()) < 1e-4      # the sticky matrix is the sticky model
    filt = h.transform(corpus, mode='filter')
    assert isinstance(filt, DeviceCorpus) and not torch.equal(filt.table, post.table)
    assert abs(h.score(corpus) - s.score(corpus)) < 1e-4
    h.fit(corpus, n_iter=3, tol=-np.inf)
    post = h.transform(corpus)
    r_raw = ABXEvaluator(items, g.transform(corpus), distance='kl').run('within')
    r = ABXEvaluator(items, post, distance='kl').run('within')
    print('ABX (kl): raw %s, transition-smoothed %s' % (r_raw, r))
    assert r.error < 50.0                 # the plumbing, not a quality claim
    path = str(tmp_path / 'dense.npz')
    h.save(path)
    assert torch.equal(hmm.TransitionHmmPosteriorgram.load(path).transform(corpus).table, post.table)
    # the command line: fit-trans from the saved model, and transform recognises a file that holds trans
    fpath, opath, ppath = str(tmp_path / 'feats.npz'), str(tmp_path / 'out.npz'), str(tmp_path / 'post.npz')
    np.savez(fpath, **feats)
    assert hmm.main(['fit-trans', path, fpath, opath, '--n-iter', '1', '--params', 'ti']) == 0
    assert hmm.main(['transform', opath, fpath, ppath]) == 0
    with np.load(ppath) as z:
        assert sorted(z.files) == sorted(feats) and all(z[k].shape == (feats[k].shape[0], 8) for k in feats)
