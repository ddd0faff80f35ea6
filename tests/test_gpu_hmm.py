"""abn_hmm_forward_backward and StickyHmmPosteriorgram on the MI355X against tests/hmm_np.py.

The error bars (all derived, none tuned).  The emission scores carry tests/test_gpu_gmm.py's score bar: with the
yardstick = the float32 numpy scores' own scaled maximum error against float64, bar = max(2^-22, 4 x yardstick), and
eps_t = bar x the frame's largest score scale.  The chain adds delta = (K + 16) 2^-24 per frame: the exp (2), the
prediction (3), the product (1), the K-term sum of positives (K - 1 at the worst), the reciprocal and its product (2),
and in the backward sweep the same count again for another frame's factor -- the kernel's count stays inside K + 16.
Perturbing every factor of every path by at most e^(+-(eps_t + delta)) moves a ratio of path sums by at most
e^(+-2 S), S = the sum of eps_t + delta over the utterance's good frames.  So
    gamma, ahat: |d| <= g64 expm1(2 S) + 2^-22;   |sum_k gamma - 1| <= expm1(2 S) + 2^-22;
    loglik: |d| <= S + 2 x 2^-24 sum_t |m_t|;     stays: |d| <= n_good expm1(2 S).
Tight checks free of the score term: rho = 0 against abn_gmm_posteriors; every utterance reversed (the chain is
reversible and a row's scores do not depend on its position: the backward sweep against the forward one); K = 1.
Each grid case prints the kernel's error over the float32 restatement's own (-s shows it).

Largest kernel / float32-restatement error ratios seen on the MI355X over all grid cases: gamma 2.54 (K = 5, D = 13,
rho = 0: kernel 2.27e-6 against 8.9e-7, 0.024 of what it is allowed), ahat 1.20, loglik 1.99 (K = 130, D = 100, rho = 0.999:
8.3e-5 against 4.2e-5 nats over 300 frames, 0.01 of the bar); the bars themselves were reached to 0.046 (gamma) and 0.031
(loglik) at most.  The tight checks: rho = 0 against abn_gmm_posteriors 0.86 of the bar (K = 5), the reversal 0.0074."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_np  # noqa: E402

pytestmark = pytest.mark.gpu

U = 2.0 ** -24
FLOOR = 2.0 ** -22
LENS = (1, 2, 127, 128, 129, 300)                       # the slab edges
KS = (1, 5, 128, 130, 257, 513, 1025, 2049)             # every per-thread column count (1, 2, 4, 8, 16) of the kernel
DS = (1, 13, 40, 100, 127)
RHOS = (0.0, 0.5, 0.9, 0.999)
RATIOS = {'gamma': 0.0, 'ahat': 0.0, 'loglik': 0.0}


def dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


def make_model(T, K, D, seed, zero_weight=None, uniform=False):
    """Frames around K centres close enough to be confused, and a model near them."""
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, D)) * (2.0 / np.sqrt(D))
    x = (centres[rng.integers(0, K, size=T)] + rng.normal(size=(T, D))).astype(np.float32)
    shift = (x.astype(np.float64).mean(axis=0) if T > 1 else np.zeros(D)).astype(np.float32)
    m = centres - shift.astype(np.float64) + 0.1 * rng.normal(size=(K, D))
    v = rng.uniform(0.5, 2.0, size=(K, D))
    w = rng.dirichlet(np.full(K, 5.0))
    if zero_weight is not None:
        w[zero_weight] = 0.0
        w /= w.sum()
    if uniform:
        w = np.full(K, 1.0 / K)
    return x, shift, w, m, v


class Case(object):
    """The device tables of a model and the float64 / float32 references of a corpus under it."""

    def __init__(self, x, shift, w, m, v, lens):
        self.x, self.lens = x, np.asarray(lens, dtype=np.int64)
        self.off = np.cumsum(self.lens) - self.lens
        self.K, self.D = m.shape
        self.xc, self.bad = gmm_np.centre(x, shift)
        self.A, self.B, self.c = gmm_np.tables(w, m, v)
        self.c0 = hmm_np.emission_offsets(m, v)
        self.w32 = w.astype(np.float32)
        self.d = dict(table=dev(x, np.float32), shift=dev(shift, np.float32), A=dev(self.A, np.float32), B=dev(self.B, np.float32),
                      c0=dev(self.c0, np.float32), w=dev(self.w32, np.float32))
        self._ref = {}

    def run(self, rho, mode='smooth', off=None, lens=None, table=None, out=None):
        from abnet3_amd import hmm
        d = self.d
        post, ll, st, ng = hmm.forward_backward(d['table'] if table is None else table, self.off if off is None else off,
                                                self.lens if lens is None else lens, d['shift'], d['A'], d['B'], d['c0'], d['w'],
                                                rho, mode, out=out)
        torch.cuda.synchronize()
        return dict(post=host(post), loglik=host(ll), stays=host(st), n_good=host(ng))

    def scores(self):
        if 's64' not in self._ref:
            s64 = gmm_np.scores(self.xc, self.bad, self.A, self.B, self.c0, np.float64)
            s32 = gmm_np.scores(self.xc, self.bad, self.A, self.B, self.c0, np.float32)
            scale = gmm_np.score_scale(self.xc, self.bad, self.A, self.B, self.c0)
            good = ~self.bad
            yard = (np.abs(s32.astype(np.float64) - s64)[good] / scale[good]).max() if good.any() else 0.0
            eps = max(FLOOR, 4.0 * yard) * scale.max(axis=1)
            self._ref.update(s64=s64, s32=s32, eps=np.where(good, eps, 0.0), delta=np.where(good, (self.K + 16) * U, 0.0))
        return self._ref

    def reference(self, rho, smooth=True):
        key = (float(rho), smooth)
        if key not in self._ref:
            r = self.scores()
            self._ref[key] = (hmm_np.corpus_fast(r['s64'], self.bad, self.off, self.lens, self.w32, rho, np.float64, smooth),
                              hmm_np.corpus_fast(r['s32'], self.bad, self.off, self.lens, self.w32, rho, np.float32, smooth))
        return self._ref[key]

    def per_utterance(self, a):
        return np.array([a[o:o + n].sum() for o, n in zip(self.off, self.lens)])

    def rows(self, per_utt):
        return np.repeat(per_utt, self.lens)


def check_against_reference(case, got, rho, smooth, tag):
    """The module docstring's bars on the posteriors, the row sums, loglik, stays and n_good; fills RATIOS."""
    r = case.scores()
    ref64, ref32 = case.reference(rho, smooth)
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
    if smooth:
        bar_st = ref64['n_good'] * np.expm1(2.0 * S)
        assert (np.abs(got['stays'] - ref64['stays']) <= bar_st).all(), (tag, np.abs(got['stays'] - ref64['stays']).max())
        assert (got['stays'] >= 0).all() and (got['stays'] <= np.maximum(ref64['n_good'] - 1, 0) + 1e-6).all()
    else:
        assert not got['stays'].any()


def grid_cases():
    """Every K with the D and rho lists cycled; the utterances are LENS, one corpus per case."""
    return [(K, DS[i % len(DS)], RHOS[(i + 1) % len(RHOS)]) for i, K in enumerate(KS)] + \
           [(130, D, RHOS[i % len(RHOS)]) for i, D in enumerate(DS)] + [(5, 13, rho) for rho in RHOS]


@pytest.fixture(scope='module')
def cases():
    cache = {}

    def get(K, D, seed=0, **kw):
        key = (K, D, seed) + tuple(sorted(kw.items()))
        if key not in cache:
            x, shift, w, m, v = make_model(int(sum(LENS)), K, D, seed=1000 * K + D + seed, **kw)
            cache[key] = Case(x, shift, w, m, v, LENS)
        return cache[key]
    return get


@pytest.mark.parametrize('K,D,rho', grid_cases())
def test_smoothed_and_filtered_on_the_shape_grid(cases, K, D, rho):
    case = cases(K, D)
    tag = 'K%d D%d rho%g' % (K, D, rho)
    check_against_reference(case, case.run(rho, 'smooth'), rho, True, tag)
    check_against_reference(case, case.run(rho, 'filter'), rho, False, tag + ' filter')
    print('largest kernel / float32-restatement ratios so far:', RATIOS)


ZERO_STAY = [(1, 1), (5, 13), (128, 40), (130, 100), (257, 127), (513, 1), (2049, 13)]


@pytest.mark.parametrize('K,D', ZERO_STAY)
def test_zero_stay_is_abn_gmm_posteriors(cases, K, D):
    """rho = 0 against abn_gmm_posteriors, free of the score term: equal weights, and abn_gmm_posteriors is given the very
    table the HMM kernel reads (c0; a constant log w added to every component moves no posterior).  Both then start from
    the same score bits, and what is left is the chain's own rounding: gamma within g (K + 16) 2^-23 + 2^-22, loglik
    within sum_t ((K + 8) 2^-24 + 2^-23 |lse_t|) of sum_t (lse_t + log w)."""
    from abnet3_amd import gmm
    case = cases(K, D, uniform=True)
    assert (case.w32 == np.float32(1.0 / K)).all()
    got = case.run(0.0)
    d = case.d
    lse, g = gmm.posteriors(d['table'], d['shift'], d['A'], d['B'], d['c0'])
    lse, g = host(lse).astype(np.float64) + np.log(np.float64(case.w32[0])), host(g).astype(np.float64)
    e_g = np.abs(got['post'] - g)
    allowed = g * (K + 16) * 2.0 ** -23 + FLOOR
    bar_ll = case.per_utterance((K + 8) * U + 2.0 ** -23 * np.abs(lse))
    e_ll = np.abs(got['loglik'] - case.per_utterance(lse))
    print('K%d D%d: gamma %.3g of its bar, loglik %.3g of its bar' % (K, D, (e_g / allowed).max(), (e_ll / bar_ll).max()))
    assert (e_g <= allowed).all(), (e_g / allowed).max()
    assert (e_ll <= bar_ll).all(), (e_ll / bar_ll).max()
    assert not got['stays'].any()


@pytest.mark.parametrize('K,D', ZERO_STAY)
def test_zero_stay_against_the_mixture_with_its_own_weights(cases, K, D):
    """The same with unequal weights against the mixture's own tables.  Here the two routes do NOT start from the same bits:
    the mixture rounds c = c0 + log w once and adds it as the GEMM's last term, the HMM adds c0 and multiplies by w32.  A
    log score differs by at most M 2^-24, M = |s| + |s0| + |c| + |c0| + 1 (the two last additions, the two tables, w32), and
    a posterior moves by at most its own component's share plus the g-weighted mean over the row: that term is added to
    the bars of the test above."""
    from abnet3_amd import gmm
    case = cases(K, D)
    got = case.run(0.0)
    d = case.d
    lse, g = gmm.posteriors(d['table'], d['shift'], d['A'], d['B'], dev(case.c, np.float32))
    lse, g = host(lse).astype(np.float64), host(g).astype(np.float64)
    s0 = case.scores()['s64']
    M = np.abs(s0 + (case.c.astype(np.float64) - case.c0)) + np.abs(s0) + np.abs(case.c) + np.abs(case.c0) + 1.0
    mean_m = (g * M).sum(axis=1)
    e_g = np.abs(got['post'] - g)
    allowed = g * ((K + 16) * 2.0 ** -23 + (M + mean_m[:, None]) * U) + FLOOR
    bar_ll = case.per_utterance((K + 8) * U + 2.0 ** -23 * np.abs(lse) + mean_m * U)
    e_ll = np.abs(got['loglik'] - case.per_utterance(lse))
    print('K%d D%d: gamma %.3g of its bar, loglik %.3g of its bar' % (K, D, (e_g / allowed).max(), (e_ll / bar_ll).max()))
    assert (e_g <= allowed).all(), (e_g / allowed).max()
    assert (e_ll <= bar_ll).all(), (e_ll / bar_ll).max()


@pytest.mark.parametrize('K,D,rho', [(5, 13, 0.5), (130, 40, 0.9), (513, 100, 0.999), (2049, 1, 0.9)])
def test_reversed_utterances_come_back_reversed(cases, K, D, rho):
    case = cases(K, D)
    got = case.run(rho)
    idx = np.concatenate([np.arange(o + n - 1, o - 1, -1) for o, n in zip(case.off, case.lens)])
    rev = case.run(rho, table=dev(case.x[idx], np.float32))
    sd = case.per_utterance(np.full(len(case.x), (K + 16) * U))
    g = got['post'].astype(np.float64)
    allowed = g * np.expm1(4.0 * case.rows(sd))[:, None] + FLOOR
    e = np.abs(rev['post'][idx].astype(np.float64) - g)
    print('K%d D%d rho%g: reversal %.3g of its bar, loglik %.3g of its bar'
          % (K, D, rho, (e / allowed).max(), (np.abs(rev['loglik'] - got['loglik']) / (2.0 * sd)).max()))
    assert (e <= allowed).all(), (e / allowed).max()
    assert (np.abs(rev['loglik'] - got['loglik']) <= 2.0 * sd).all()
    assert np.array_equal(rev['n_good'], got['n_good'])


@pytest.mark.parametrize('rho', RHOS)
def test_one_component_gives_exactly_one(cases, rho):
    """K = 1: bt = 1, and for these stays (0, or >= 1/2, where 1 - rho is exact in fp32) rho + (1 - rho) = 1 exactly."""
    case = cases(1, 13)
    for mode in ('smooth', 'filter'):
        got = case.run(rho, mode)
        assert (got['post'] == 1.0).all()
    assert np.array_equal(got['n_good'], case.lens)


def test_two_calls_and_every_utterance_alone_give_the_same_bits(cases):
    case = cases(257, 40)
    a, b = case.run(0.9), case.run(0.9)
    for k in a:
        assert np.array_equal(a[k], b[k]), k
    f = case.run(0.9, 'filter')
    for u, (o, n) in enumerate(zip(case.off, case.lens)):
        for mode, whole in (('smooth', a), ('filter', f)):
            one = case.run(0.9, mode, off=[0], lens=[n], table=dev(case.x[o:o + n], np.float32))
            assert np.array_equal(one['post'], whole['post'][o:o + n]), (u, mode)
            assert one['loglik'][0] == whole['loglik'][u] and one['stays'][0] == whole['stays'][u] and one['n_good'][0] == n


def test_more_utterances_than_workgroups():
    """300 utterances of 1 .. 5 frames: the persistent loop; every utterance as in the restatement, and in any order."""
    rng = np.random.default_rng(9)
    lens = rng.integers(1, 6, size=300)
    x, shift, w, m, v = make_model(int(lens.sum()), 5, 13, seed=9)
    case = Case(x, shift, w, m, v, lens)
    got = case.run(0.9)
    check_against_reference(case, got, 0.9, True, '300 utterances')
    perm = rng.permutation(300)
    other = case.run(0.9, off=case.off[perm], lens=case.lens[perm])
    assert np.array_equal(other['post'], got['post'])
    assert np.array_equal(other['loglik'], got['loglik'][perm]) and np.array_equal(other['stays'], got['stays'][perm])


def test_bad_rows_are_zero_counted_and_passed_over():
    x, shift, w, m, v = make_model(int(sum(LENS)), 130, 39, seed=4)
    rows = [0, 3, 130, 257, 258, 400, 686]               # (utterances start at 0, 1, 3, 130, 258, 387)
    xb = x.copy()
    xb[0, 3], xb[3, 0], xb[130, 38], xb[257, :], xb[258, 5], xb[400, 7], xb[686, 1] = np.nan, np.inf, -np.inf, np.nan, 3e19, np.inf, np.nan
    case = Case(xb, shift, w, m, v, LENS)
    assert list(np.flatnonzero(case.bad)) == rows        # 3e19: the overflow of xc^2
    got = case.run(0.9)
    check_against_reference(case, got, 0.9, True, 'bad rows')
    assert not got['post'][rows].any()
    assert list(got['n_good']) == [0, 2, 126, 126, 128, 298]
    assert got['loglik'][0] == 0.0 and got['stays'][0] == 0.0
    # passed over: the table without the rows gives the other rows' bits (loglik: the blocks of its float64 sum move)
    keep = np.setdiff1d(np.arange(len(x)), rows)
    lens2 = [2, 126, 126, 128, 298]                      # (the first utterance was its BAD frame alone)
    clean = Case(xb[keep], shift, w, m, v, lens2).run(0.9)
    assert np.array_equal(clean['post'], got['post'][keep])
    assert np.array_equal(clean['n_good'], got['n_good'][1:])
    assert np.abs(clean['loglik'] - got['loglik'][1:]).max() <= 1e-12 * np.abs(got['loglik']).max()
    assert np.array_equal(clean['stays'], got['stays'][1:])


def test_a_component_of_weight_zero_keeps_gamma_zero(cases):
    case = cases(130, 13, zero_weight=7)
    assert case.w32[7] == 0.0 and np.isfinite(case.c0[7])
    for mode in ('smooth', 'filter'):
        got = case.run(0.9, mode)
        assert not got['post'][:, 7].any()
        check_against_reference(case, got, 0.9, mode == 'smooth', 'zero weight ' + mode)


def test_utterances_outside_the_table_and_refusals(cases):
    """Straight at the library: a bad off / len marks its utterance and touches nothing; rows outside every utterance keep
    what they held; the refusals return their codes before any launch."""
    from abnet3_amd import _lib
    lib = _lib.load()
    case = cases(5, 13)
    d, T, K, D = case.d, len(case.x), 5, 13
    off = np.array([0, -1, 10, T - 3, 30], dtype=np.int64)
    lens = np.array([5, 4, -2, 4, 300], dtype=np.int32)          # fine, off < 0, len < 0, past the end, longer than the workspace holds
    post = torch.full((T, K), 7.0, dtype=torch.float32, device='cuda')
    ll = torch.zeros(5, dtype=torch.float64, device='cuda')
    st = torch.zeros(5, dtype=torch.float64, device='cuda')
    ng = torch.zeros(5, dtype=torch.int32, device='cuda')
    need = lib.abn_hmm_ws_bytes(5, 100, K, D)
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    off_d, len_d = dev(off, np.int64), dev(lens, np.int32)
    p = _lib.ptr

    def call(**kw):
        a = dict(x=p(d['table']), T=T, D=D, off=p(off_d), len=p(len_d), n=5, shift=p(d['shift']), A=p(d['A']),
                 B=p(d['B']), c0=p(d['c0']), w=p(d['w']), K=K, rho=0.5, mode=0, post=p(post), ll=p(ll), st=p(st), ng=p(ng), ws=p(ws),
                 bytes=need, stream=_lib.stream())
        a.update(kw)
        return lib.abn_hmm_forward_backward(*a.values())
    assert call() == 0
    torch.cuda.synchronize()
    got, gll, gng = host(post), host(ll), host(ng)
    assert list(gng) == [5, -1, -1, -1, -1] and np.isfinite(gll[0]) and np.isnan(gll[1:]).all() and np.isnan(host(st)[1:]).all()
    assert (got[5:] == 7.0).all() and np.abs(got[:5].sum(axis=1) - 1.0).max() < 1e-5
    alone = case.run(0.5, off=[0], lens=[5])
    assert np.array_equal(alone['post'][:5], got[:5]) and alone['loglik'][0] == gll[0]
    before = post.clone()
    assert call(rho=1.0) == _lib.E_ARG and call(rho=float('nan')) == _lib.E_ARG and call(mode=3) == _lib.E_ARG
    assert call(post=None) == _lib.E_ARG and call(T=0) == _lib.E_ARG
    assert call(K=lib.abn_hmm_max_k() + 1) == _lib.E_UNSUPPORTED and call(D=lib.abn_gmm_max_d() + 1) == _lib.E_UNSUPPORTED
    assert call(bytes=5 * 128 * 128 * 4) == _lib.E_WORKSPACE and call(ws=None) == _lib.E_WORKSPACE
    torch.cuda.synchronize()
    assert torch.equal(post, before)


# ---- end to end --------------------------------------------------------------------------------------------------------
def planted_model(seed=0):
    from abnet3_amd.gmm import GmmPosteriorgram
    x, lens, w, mu = hmm_np.planted(seed)
    g = GmmPosteriorgram(4)
    g.weights_, g.means_, g.variances_ = w.astype(np.float64), mu.astype(np.float64), np.ones_like(mu)
    g.shift_, g.gv_ = x.astype(np.float64).mean(axis=0).astype(np.float32), np.ones(3)
    return g, x, lens


def test_fit_stay_recovers_the_planted_stay():
    from abnet3_amd.hmm import StickyHmmPosteriorgram
    g, x, lens = planted_model(0)
    feats = {'u%03d' % i: x[o:o + n] for i, (o, n) in enumerate(zip(np.cumsum(lens) - lens, lens))}
    h = StickyHmmPosteriorgram(g, 0.5).fit_stay(feats, n_iter=10, tol=-np.inf)
    print('fit_stay: %.4f, log-likelihoods %s' % (h.stay_, ' '.join('%.5f' % v for v in h.log_likelihoods)))
    assert abs(h.stay_ - 0.9) <= 0.02 and len(h.log_likelihoods) == 10 and h.n_bad_ == 0
    # non-decreasing within the loglik bar (per good frame): the score bar and the chain's delta of every frame
    case = Case(x, g.shift_, g.weights_, g.means_ - g.shift_.astype(np.float64), g.variances_, lens)
    r = case.scores()
    m = np.where(case.w32 > 0, r['s64'], -np.inf).max(axis=1)
    bar = float((r['eps'] + r['delta'] + 2.0 * U * np.abs(m)).sum() / len(x))
    assert (np.diff(h.log_likelihoods) >= -2.0 * bar).all(), (np.diff(h.log_likelihoods), bar)
    # (2 bar: each of the two likelihoods of a difference carries the bar)
    utts = [(r['s64'][o:o + n], case.bad[o:o + n]) for o, n in zip(case.off, case.lens)]
    assert abs(h.score(feats) - hmm_np.em_stay(utts, case.w32, h.stay_, n_iter=1)[1][0] / len(x)) <= bar


def test_transform_of_a_corpus_and_downstream(tmp_path):
    from abnet3_amd import gmm, hmm
    from abnet3_amd.abx import ABXEvaluator, kl_tables
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=60, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    g = gmm.GmmPosteriorgram(8, n_iter=10).fit(corpus)
    h = hmm.StickyHmmPosteriorgram(g, 0.8)
    post = h.transform(corpus)
    assert isinstance(post, DeviceCorpus) and post.names == corpus.names and post.dim == 8 and post.total == corpus.total
    for k in corpus.names:
        assert post.length[k] == corpus.length[k] and post.offset[k] == corpus.offset[k]
        assert np.array_equal(post.times[k], corpus.times[k])
    assert torch.equal(h.transform(feats), post.table)                            # the dict form: row for row
    assert int(kl_tables(post.table).bad.sum().item()) == 0
    assert abs(float(post.table.sum(dim=1).mean().item()) - 1.0) < 1e-5
    raw = g.transform(corpus)
    zero = hmm.StickyHmmPosteriorgram(g, 0.0).transform(corpus)
    assert float((zero.table - raw.table).abs().max().item()) < 1e-4              # rho = 0 is the mixture
    assert not torch.equal(post.table, raw.table)
    filt = h.transform(corpus, mode='filter')
    assert isinstance(filt, DeviceCorpus) and not torch.equal(filt.table, post.table)
    r_raw = ABXEvaluator(items, raw, distance='kl').run('within')
    r = ABXEvaluator(items, post, distance='kl').run('within')
    print('ABX (kl): raw %s, smoothed %s' % (r_raw, r))
    assert r.error < 50.0                 # the plumbing, not a quality claim
    path = str(tmp_path / 'hmm.npz')
    h.save(path)
    assert torch.equal(hmm.StickyHmmPosteriorgram.load(path).transform(corpus).table, post.table)
