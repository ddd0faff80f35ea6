"""Sparse transitions and far-apart emissions on the host: tests/hmm_range_np.py's builders, the float64 restatements against
enumeration of all paths at the floors, the invariants on the float64 restatement of every grid case, and the
classification of the grid into in range / in the window, pinned.  No kernel runs here.

The classification as computed (N_UTT = 8 utterances a case; a case is in range when all of them are; -s prints the count
and the float32 restatement's worst error over its bar for every case).  Window gaps of the grid 20, 60, 90, 120, 160, 300:

    matrix          K = 4, L = 24           K = 65, L = 300                 K = 128, L = 140
                    2^-80      2^-100       2^-80          2^-100           2^-80        2^-100
    cyclic          120        120          60 120         20 60 90 120     60           20 60 120
    left_to_right   60 120     60 120       60 120         20 60 90 120     60 120       20 60 120
    blocks          120        120          60 120         20 60 90 120     60 120       20 60 90
    counts          -          -            60 90 120      60 90 120        60           60 120

103 cases are in range (the eight moved ones of hmm_range_np.MOVED included), 49 in the window.  In the window the float32
restatement's gamma is off by up to 4.2e6 bars or not finite (all matrices but `counts` at K >= 65, 2^-100, gaps 60 and 90),
its loglik by up to 3.9e4 bars.  Gaps 160 and 300 are in range everywhere: the off-state emissions are exact zeros and the
chain is a product of floors and ones.  A gap of 20 at K >= 65 holds misses of 40, 60 and 80 nats (the other code words) and
is in the window at the floor 2^-100.

The sticky chain on tiny_weights (components at 2^-79 .. 2^-60, some retired): a window exists.  K = 65 and 128 at gap 60 with
stay 0.9 and 1 - 2^-20 (gamma up to 3.5e3 bars, loglik up to 192), K = 65 at gap 20 with stay 1 - 2^-20 (gamma 20 bars); K = 128
at gap 20, stay 1 - 2^-20 sits at the bar (1.04).  Stay 0, K = 4 and the gaps from 90 on are in range."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_bw_np  # noqa: E402
import hmm_dense_np as dn  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_np  # noqa: E402
import hmm_range_np as hr  # noqa: E402


# ---- the builders --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K', [4, 65, 128, 256])
def test_code_words_give_the_stated_gaps(K):
    mu = hr.means(K, 60.0)
    d2 = ((mu[:, None, :] - mu[None, :, :]) ** 2).sum(axis=2) / 2.0
    off = d2[~np.eye(K, dtype=bool)]
    assert np.abs(off.min() - 60.0) <= 1e-9 and set(np.round(off / 60.0).astype(int)) <= {1, 2, 3, 4}
    assert np.abs(np.abs(off / 60.0 - np.round(off / 60.0))).max() <= 1e-12
    assert np.abs((mu * mu).sum(axis=1) - 120.0).max() <= 1e-9


@pytest.mark.parametrize('name', hr.MATRICES)
@pytest.mark.parametrize('K', [4, 65, 128])
@pytest.mark.parametrize('e', hr.EPS_EXP)
def test_matrix_builders_hold_the_floor_exactly_and_pass_the_models_checks(name, K, e):
    from abnet3_amd import hmm
    eps = 2.0 ** -e
    states = np.concatenate([hr.planted_states(np.random.default_rng(u), K, 24) for u in range(3)])
    init, trans = hr.transitions(name, K, eps, states, np.full(3, 24))
    assert init.dtype == np.float32 and trans.dtype == np.float32 and trans.flags['C_CONTIGUOUS']
    i32, t32 = hmm.check_transitions('test', init, trans)                      # finite, >= 2^-100, sums within 1e-3
    assert np.array_equal(i32, init) and np.array_equal(t32, trans)
    at_floor = (trans == np.float32(eps)).sum(axis=1)
    assert trans.min() == np.float32(eps)
    if name == 'counts':                                                       # a row with a count is sparse, one without is uniform
        seen = hr.counts_of(states, np.full(3, 24), K)[0].sum(axis=1) > 0
        assert (at_floor[seen] >= K - 4).all() and seen.any() and not at_floor[~seen].any()
    else:
        assert (at_floor >= K - 4).all()
    assert (init == np.float32(eps)).any() == (name != 'cyclic')
    li, lt = hmm.log_transitions(init, trans)
    assert lt.min() == np.float32(-e * np.log(2.0)) and np.isfinite(li).all()
    if name == 'counts' and e == 80:                                           # the model's own M-step gives this matrix
        xi, first = hr.counts_of(states, np.full(3, 24), K)
        uni_t, uni_i = np.full((K, K), 1.0 / K), np.full(K, 1.0 / K)
        t64, i64 = hmm.transition_update(np.concatenate([xi, first[None, :]]), uni_t, uni_i, alpha=0.0)
        assert np.array_equal(t64.astype(np.float32), trans) and np.array_equal(i64.astype(np.float32), init)
        t_np, i_np = dn.mstep(xi, first, uni_t, uni_i, 0.0)
        assert np.array_equal(t_np, t64) and np.array_equal(i_np, i64)


def test_planted_sequences_force_about_half_the_transitions_through_the_floor():
    c = hr.dense_case('cyclic', 65, 300, 80, 60)
    n_floor = n_all = 0
    for o, n in zip(c.off, c.lens):
        s = c.states[o:o + n]
        n_floor += int((c.trans[s[:-1], s[1:]] == np.float32(2.0 ** -80)).sum())
        n_all += n - 1
    assert 0.4 <= n_floor / n_all <= 0.6
    again = hr.dense_case('cyclic', 65, 300, 80, 60)                           # deterministic
    assert np.array_equal(again.x, c.x) and np.array_equal(again.trans, c.trans)


def test_tiny_weights_hold_tiny_and_retired_components():
    for K in (4, 65, 128):
        w = hr.tiny_weights(K, K)
        w32 = w.astype(np.float32)
        tiny = (w32 > 0) & (w32 < 2.0 ** -59)
        assert abs(w.sum() - 1.0) <= 1e-12 and tiny.sum() >= K // 4 and (w32 == 0).sum() >= max(1, K // 10)
        assert w32[tiny].min() >= 2.0 ** -79 and w32[w32 > 0].min() * 2.0 ** -20 >= 2.0 ** -100      # check_stay's condition


def test_the_filtered_references_are_the_smoothed_runs_ahat():
    c = hr.dense_case('blocks', 4, 24, 100, 60, bad_rows=(0, 30, 47))
    r = c.scores()
    for (dt, s), mine in zip(((np.float64, r['s64']), (np.float32, r['s32'])), c.reference(False)):
        want = dn.corpus(s, c.bad, c.off, c.lens, c.init, c.trans, dt, smooth=False)
        for k in ('post', 'ahat', 'm', 'loglik', 'n_good', 'xi', 'first'):
            assert np.array_equal(mine[k], want[k]), k


# ---- the yardsticks at the floors ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('name', hr.MATRICES)
@pytest.mark.parametrize('e', hr.EPS_EXP)
def test_dense_restatement_equals_enumeration_on_a_sparse_case(name, e):
    """K = 3, 6 frames, every planted transition of one utterance: the float64 restatement against all 3^6 paths.  The
    enumeration adds path weights that differ by 2^-100 and more in one float64 sum: what is below 2^-52 of the total is
    lost there, so the comparison is relative to the total (1e-12), and loglik, a sum of logs, is compared absolutely."""
    for gap in (20, 90, 300):
        c = hr.dense_case(name, 3, 6, e, gap, n_utt=4, bad_rows=(8,))
        s64 = c.scores()['s64']
        for o, n in zip(c.off, c.lens):
            sl = slice(o, o + n)
            gamma, ll, xi, first = dn.brute_force(s64[sl], c.bad[sl], c.init, c.trans)
            for fb in (dn.forward_backward, dn.forward_backward_fast):
                r = fb(s64[sl], c.bad[sl], c.init, c.trans)
                assert np.abs(r['gamma'] - gamma).max() <= 1e-12 and abs(r['loglik'] - ll) <= 1e-9 * (1.0 + abs(ll))
                assert np.abs(r['xi'] - xi).max() <= 1e-12 and np.abs(r['first'] - first).max() <= 1e-12
                assert r['n_good'] == int((~c.bad[sl]).sum())


@pytest.mark.parametrize('stay', hr.STAYS)
def test_sticky_restatements_equal_enumeration_with_tiny_and_retired_weights(stay):
    for gap in (20, 90, 300):
        c = hr.sticky_case(4, 6, gap, n_utt=3, bad_rows=(7,))
        assert (c.w32 == 0).sum() == 1 and ((c.w32 > 0) & (c.w32 < 2.0 ** -59)).sum() == 1
        s64 = c.scores()['s64']
        for o, n in zip(c.off, c.lens):
            sl = slice(o, o + n)
            gamma, ll, stays = hmm_np.brute_force(s64[sl], c.bad[sl], c.w32, stay)
            slow = hmm_np.forward_backward(s64[sl], c.bad[sl], c.w32, stay)
            fast = hmm_np.forward_backward_fast(s64[sl], c.bad[sl], c.w32, stay)
            bw = hmm_bw_np.forward_backward(s64[sl], c.bad[sl], c.w32, stay)
            for g, l, s in ((slow['gamma'], slow['loglik'], slow['stays']), (fast[3], fast[0], fast[1]), (bw['gamma'], bw['loglik'], bw['stays'])):
                assert np.isfinite(g).all() and np.abs(g - gamma).max() <= 1e-12
                assert abs(l - ll) <= 1e-9 * (1.0 + abs(ll)) and abs(s - stays) <= 1e-12 * n
            sk, draws = hmm_bw_np.brute_force(s64[sl], c.bad[sl], c.w32, stay)
            assert np.abs(bw['stay_k'] - sk).max() <= 1e-12 and np.abs(bw['draws'] - draws).max() <= 1e-12
            # a far emission at the retired component: exp overflows there in float32, and the restatement must not see it
            r32 = hmm_np.forward_backward(c.scores()['s32'][sl], c.bad[sl], c.w32, stay, np.float32)
            assert np.isfinite(r32['gamma']).all() and not r32['gamma'][:, c.w32 == 0].any()


# ---- the grid ------------------------------------------------------------------------------------------------------------
def check_invariants_f64(c):
    ref64 = c.reference(True)[0]
    li, lt = c.log_tables()
    s64 = c.scores()['s64']
    opt = np.array([dv.optimum_f64(s64[o:o + n], ~c.bad[o:o + n], li, lt) for o, n in zip(c.off, c.lens)])
    slack = 1e-9 * (1.0 + np.abs(opt)) + 2.0 ** -24 * dv.table_max(li, lt) * ref64['n_good']      # (the log tables' one rounding)
    for post in (ref64['post'], ref64['ahat']):
        v = hr.violations(c, post, ref64['loglik'], np.concatenate([ref64['xi'], ref64['first'][None, :]]), opt, slack, ref64['n_good'])
        assert v == [], (c.tag, v)
    assert abs(ref64['xi'].sum() - np.maximum(ref64['n_good'] - 1, 0).sum()) <= 1e-9 * ref64['n_good'].sum()


@pytest.mark.parametrize('name', hr.MATRICES)
@pytest.mark.parametrize('K,L', hr.SHAPES)
def test_the_grid_is_classified_as_pinned_and_the_float64_restatement_keeps_the_invariants(name, K, L):
    for e in hr.EPS_EXP:
        for gap in hr.GAPS:
            c = hr.dense_case(name, K, L, e, gap)
            check_invariants_f64(c)
            ok = hr.classify(c)
            r32 = c.reference(True)[1]
            er = hr.dense_errors(c, r32['post'], r32['ahat'], r32['loglik'], r32['xi_utt'], r32['first_utt'])
            print('%s: %d of %d utterances in range; float32 restatement over its bars: %s'
                  % (c.tag, ok.sum(), len(ok), ' '.join('%s %.3g' % (k, v.max()) for k, v in er.items())))
            assert bool(ok.all()) == (gap not in hr.WINDOW[(name, K, e)]), (c.tag, ok)


def test_the_moved_cases_are_in_range_and_the_listed_ones_are_not():
    for name, K, L, e, listed, taken in hr.MOVED:
        assert listed in hr.WINDOW[(name, K, e)]
        c = hr.dense_case(name, K, L, e, taken)
        check_invariants_f64(c)
        assert hr.classify(c).all(), c.tag


def test_the_in_range_cases_with_bad_rows_are_in_range():
    for name, K, L, e, gap in hr.BAD_IN_RANGE:
        c = hr.dense_case(name, K, L, e, gap, bad_rows=hr.bad_rows_for(L))
        assert list(np.flatnonzero(c.bad)) == list(hr.bad_rows_for(L)) and (name, K, L, e, gap) in hr.in_range_cases()
        check_invariants_f64(c)
        assert hr.classify(c).all(), c.tag


def test_the_in_range_list_is_long_enough_and_covers_every_k():
    cases = hr.in_range_cases()
    assert len(set(cases)) == len(cases) and not set(cases) & set(hr.window_cases())
    for e in hr.EPS_EXP:
        mine = [c for c in cases if c[3] == e]
        assert len(mine) >= 12 and {c[1] for c in mine} == {4, 65, 128} and {c[0] for c in mine} == set(hr.MATRICES)
        assert all((n, K, L, e, 300) in mine for n in hr.MATRICES for K, L in hr.SHAPES)
    assert all((n, K, L, 80, 160) in cases for n in hr.MATRICES for K, L in hr.SHAPES)


@pytest.mark.parametrize('K,L', hr.SHAPES)
def test_the_sticky_grid_is_classified_as_recorded(K, L):
    for gap in hr.GAPS:
        c = hr.sticky_case(K, L, gap)
        for i, stay in enumerate(hr.STAYS):
            ref64, r32 = c.reference(stay, True)
            assert np.isfinite(ref64['post']).all() and (ref64['post'] >= 0).all() and np.isfinite(ref64['loglik']).all()
            assert np.abs(ref64['post'].sum(axis=1) - 1.0).max() <= 1e-9 and not ref64['post'][:, c.w32 == 0].any()
            ok = hr.classify_sticky(c, stay)
            er = hr.sticky_errors(c, stay, r32['post'], r32['ahat'], r32['loglik'], r32['stays'])
            print('%s stay %.7g: %d of %d utterances in range; float32 restatement over its bars: %s'
                  % (c.tag, stay, ok.sum(), len(ok), ' '.join('%s %.3g' % (k, v.max()) for k, v in er.items())))
            if (K, gap, i) not in hr.STICKY_EDGE:
                assert bool(ok.all()) == ((K, gap, i) not in hr.STICKY_WINDOW), (c.tag, stay, ok)
    for stay in hr.STAYS:                                                     # the GPU test's gap-300 cases carry BAD rows
        assert hr.classify_sticky(hr.sticky_case(K, L, 300, bad_rows=hr.bad_rows_for(L)), stay).all()
