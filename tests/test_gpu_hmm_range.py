"""The HMM chains on the MI355X with sparse transitions (floors 2^-80 and 2^-100) and emissions 10 to 300 nats apart:
tests/hmm_range_np.py's cases, classified by tests/test_hmm_range_host.py from the restatements alone.

In range (the float32 restatement meets the bars): abny_hmm_dense_forward_backward, smoothed with the statistics and
filtered, must meet tests/test_gpu_hmm_dense.py's bars through its check_against_reference, unchanged, and the invariants
of hmm_range_np.violations, the sandwich against abnz_hmm_dense_viterbi's log_prob among them; the sticky chain
(abn_hmm_forward_backward, abn_hmm_forward_backward_stats, abn_hmm_accumulate on its table) must meet tests/test_gpu_hmm.py's
and tests/test_gpu_hmm_bw.py's bars on weights that hold components at 2^-79 .. 2^-60 and retired ones.  These cases reach
exact-zero emissions, c_t at the floor and bhat above 2^80.

The decoders run in the log domain, where a floor is -55.45 or -69.31 beside 0, and must not notice: on integer scores and
power-of-two tables every one EQUALS its restatement (ties at the floor included), on the float cases -- in range or not -- it
is within its documented allowance of the float64 optimum.

In the window nothing is asserted of the values: what the chains return there is undefined today.  Each case runs once; its
shape, n_good and the zero rows at BAD frames are checked, and the device's error over the bar is printed beside the
float32 restatement's, with the invariants the device breaks (-s shows it).  The yardstick for work that widens the range
is the float64 restatement under the unchanged bars, never these figures.

RECORDED below holds the largest figures a full run of this file printed on the MI355X."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_bw_np  # noqa: E402
import hmm_dense_dur_np as dd  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_hsmm_np as hs  # noqa: E402
import hmm_range_np as hr  # noqa: E402
import hmm_vit_np  # noqa: E402
import test_gpu_hmm as sticky_file  # noqa: E402
from test_gpu_hmm import FLOOR, U, dev, host  # noqa: E402
from test_gpu_hmm_bw import frames_per_range  # noqa: E402
from test_gpu_hmm_dense import check_against_reference  # noqa: E402

pytestmark = pytest.mark.gpu

RECORDED = ('in range, full-transition chain (107 cases, 4 of them with BAD rows, each smoothed and filtered): gamma 0.571 of its bar '
            '(left_to_right, K = 65, 2^-80, gap 90), ahat 0.012, loglik 0.074, xi 0.022, first 0.040; every invariant held, the sandwich '
            'included.  In range, sticky chain (48 cases): gamma 0.013, ahat 0.0098, loglik 0.057, stays 6.0e-4, stay_k 1.2e-3, '
            'abn_hmm_accumulate 9.6e-4 of their bars.  The decoders used at most 0.0045 of their allowance on the float cases and '
            'equalled their restatements on the exact ones.  '
            'In the window, full-transition chain (49 cases, each with three BAD rows): the device follows the float32 restatement, '
            'denormals included (error over the bar, device / restatement: gamma inf / inf, ahat 4.19e6 / 4.19e6, loglik 3.92e4 / 3.92e4, '
            'xi inf / inf, first inf / inf; per case the two agree to the digits printed, but for ahat where both are below 1e-6 of the '
            'bar); it kept no case wholly inside the bars and in every case as many utterances inside as the restatement.  12 cases gave '
            'non-finite posteriors, negative entries and negative xi (all four matrices at the floor 2^-100, gaps 60 and 90, K >= 65), 29 '
            'broke the row sums, 23 the sandwich (every case at 2^-100 with gaps 60 .. 120 that lost loglik; none at 2^-80, where '
            'loglik stays within 7.8 bars), 10 broke no invariant although gamma was off by 1.5 to 240 bars (2^-80, gaps 90 and 120).  In the '
            'window, sticky chain (6 cases): gamma 3.51e3 / 3.51e3, ahat 3.10e3 / 3.10e3, loglik 192 / 192, stays 887 / 887; finite and '
            'non-negative everywhere, the row sums broken at stay 1 - 2^-20, gap 60.')

WORST = {}                                                # the largest figures of this run, printed by every test that adds to them


def note(key, value):
    if np.isnan(value) or value > WORST.get(key, -1.0):
        WORST[key] = float(value)


def case_id(c):
    return '%s-K%d-L%d-2^-%d-gap%d' % c


# ---- the full-transition chain, in range ---------------------------------------------------------------------------------
def decode(case, min_duration=1):
    from abnet3_amd import hmm
    d = case.d
    li, lt = hmm.log_transitions(case.init, case.trans)
    out = hmm.dense_viterbi(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], dev(li, np.float32), dev(lt, np.float32),
                            min_duration=min_duration)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out), li, lt


def check_in_range(case):
    ref64 = case.reference(True)[0]
    smooth, filt = case.run('smooth'), case.run('filter')
    assert smooth['post'].shape == (len(case.x), case.K) and smooth['stats'].shape == (case.K + 1, case.K)
    (ids, lp, nsw, ng), li, lt = decode(case)
    assert np.array_equal(ng, ref64['n_good']) and np.array_equal(ids < 0, case.bad)
    slack = 2.0 * hr.decoder_delta(case, li, lt) + hr.loglik_bar(case, ref64['m'])
    for got in (smooth, filt):
        v = hr.violations(case, got['post'], got['loglik'], got['stats'], lp, slack, ng)
        assert v == [], (case.tag, v)
    check_against_reference(case, smooth, True, case.tag)
    check_against_reference(case, filt, False, case.tag + ' filter')
    e = hr.dense_errors(case, smooth['post'], filt['post'], smooth['loglik'])
    xi, first = hr.corpus_stats_error(case, smooth['stats'])
    for k, val in (('gamma', e['gamma'].max()), ('ahat', e['ahat'].max()), ('loglik', e['loglik'].max()), ('xi', xi), ('first', first)):
        note('in range, dense: %s over its bar' % k, val)
    lo = (smooth['loglik'] - (lp - slack)).min()
    hi = (lp + ng * np.log(case.K) + slack - smooth['loglik']).min()
    print('%s: the sandwich holds with %.3g nats to spare below and %.3g above (slack %.3g)' % (case.tag, lo, hi, slack.max()))
    # what these cases were built to reach
    c_floor = np.exp((smooth['loglik'] - case.per_utterance(ref64['m'])) / np.maximum(ng, 1)).min()
    print('%s: geometric mean of c_t per utterance down to 2^%.1f; exact zeros in the posteriors: %d of %d'
          % (case.tag, np.log2(c_floor), int((smooth['post'][~case.bad] == 0).sum()), smooth['post'][~case.bad].size))
    print('largest figures so far:', WORST)


@pytest.mark.parametrize('c', hr.in_range_cases(), ids=case_id)
def test_dense_chain_in_range_meets_the_bars_and_the_invariants(c):
    check_in_range(hr.dense_case(*c))


@pytest.mark.parametrize('c', hr.BAD_IN_RANGE, ids=case_id)
def test_dense_chain_in_range_with_bad_rows(c):
    case = hr.dense_case(*c, bad_rows=hr.bad_rows_for(c[2]))
    check_in_range(case)
    assert list(case.run('smooth')['n_good']) == [c[2] - 1, c[2] - 2] + [c[2]] * (hr.N_UTT - 2)


# ---- the full-transition chain, in the window ------------------------------------------------------------------------------
@pytest.mark.parametrize('c', hr.window_cases(), ids=case_id)
def test_dense_chain_in_the_window_is_run_and_reported(c):
    case = hr.dense_case(*c, bad_rows=hr.bad_rows_for(c[2]))
    ref64, ref32 = case.reference(True)
    smooth, filt = case.run('smooth'), case.run('filter')
    for got in (smooth, filt):
        assert got['post'].shape == (len(case.x), case.K) and got['loglik'].shape == (hr.N_UTT,) and got['stats'].shape == (case.K + 1, case.K)
        assert np.array_equal(got['n_good'], ref64['n_good']) and not got['post'][case.bad].any()
    (ids, lp, nsw, ng), li, lt = decode(case)
    slack = 2.0 * hr.decoder_delta(case, li, lt) + hr.loglik_bar(case, ref64['m'])
    mine = hr.dense_errors(case, smooth['post'], filt['post'], smooth['loglik'])
    theirs = hr.dense_errors(case, ref32['post'], ref32['ahat'], ref32['loglik'])
    mine['xi'], mine['first'] = hr.corpus_stats_error(case, smooth['stats'])
    theirs['xi'], theirs['first'] = hr.corpus_stats_error(case, np.concatenate([ref32['xi'], ref32['first'][None, :]]))
    broken = hr.violations(case, smooth['post'], smooth['loglik'], smooth['stats'], lp, slack, ng)
    ok_dev = np.all([mine[k] <= 1.0 for k in ('gamma', 'ahat', 'loglik')], axis=0)
    print('%s (with BAD rows): error over the bar, device / float32 restatement: %s; utterances inside the bars: device %d, restatement %d of %d; '
          'invariants the device breaks: %s' % (case.tag, ', '.join('%s %.3g / %.3g' % (k, np.max(mine[k]), np.max(theirs[k])) for k in mine),
                                                ok_dev.sum(), np.all([theirs[k] <= 1.0 for k in ('gamma', 'ahat', 'loglik')], axis=0).sum(),
                                                hr.N_UTT, broken or 'none'))
    for k in mine:
        note('window, dense: device %s over its bar' % k, np.max(mine[k]))
        note('window, dense: float32 restatement %s over its bar' % k, np.max(theirs[k]))
    for b in broken:
        WORST['window, dense: cases that break "%s"' % b] = WORST.get('window, dense: cases that break "%s"' % b, 0) + 1
    WORST['window, dense: cases run'] = WORST.get('window, dense: cases run', 0) + 1
    WORST['window, dense: cases the device keeps inside the bars'] = WORST.get('window, dense: cases the device keeps inside the bars', 0) + int(ok_dev.all())
    print('largest figures so far:', WORST)


# ---- the sticky chain ------------------------------------------------------------------------------------------------------
def sticky_id(c):
    return 'K%d-L%d-gap%d-stay%d' % c


def sticky_runs(case, stay):
    from abnet3_amd import hmm
    d = case.d
    post, ll, st, ng, sk = hmm.forward_backward(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], d['w'], stay, 'smooth',
                                                want_stay_k=True)
    sums = hmm.accumulate(d['table'], post, d['shift'], 0)
    torch.cuda.synchronize()
    stats = dict(post=host(post), loglik=host(ll), stays=host(st), n_good=host(ng), stay_k=host(sk), sums=host(sums))
    return stats, case.run(stay, 'smooth'), case.run(stay, 'filter')


IN_STICKY = [c for c in hr.sticky_grid() if (c[0], c[2], c[3]) not in hr.STICKY_WINDOW + hr.STICKY_EDGE]
OUT_STICKY = [c for c in hr.sticky_grid() if (c[0], c[2], c[3]) in hr.STICKY_WINDOW + hr.STICKY_EDGE]


@pytest.mark.parametrize('c', IN_STICKY, ids=sticky_id)
def test_sticky_chain_in_range_meets_the_bars(c):
    K, L, gap, i = c
    stay = hr.STAYS[i]
    case = hr.sticky_case(K, L, gap, bad_rows=hr.bad_rows_for(L) if gap == 300 else ())
    stats, smooth, filt = sticky_runs(case, stay)
    for k in smooth:                                                         # the statistics entry gives the plain entry's bits
        assert np.array_equal(stats[k], smooth[k]), k
    sticky_file.check_against_reference(case, smooth, stay, True, case.tag)
    sticky_file.check_against_reference(case, filt, stay, False, case.tag + ' filter')
    dead = case.w32 == 0
    assert dead.any() and not smooth['post'][:, dead].any() and not filt['post'][:, dead].any() and (smooth['post'] >= 0).all()
    # stay_k: tests/test_gpu_hmm_bw.py's bar n_good expm1(2 S) against the float64 restatement, and its sum against `stays`
    r = case.scores()
    S = case.per_utterance(r['eps'] + r['delta'])
    bar = smooth['n_good'] * np.expm1(2.0 * S)
    ref_sk = np.array([hmm_bw_np.forward_backward(r['s64'][o:o + n], case.bad[o:o + n], case.w32, stay)['stay_k']
                       for o, n in zip(case.off, case.lens)])
    sk = stats['stay_k']
    assert np.isfinite(sk).all() and (sk >= 0).all() and not sk[:, dead].any()
    assert (np.abs(sk - ref_sk) <= bar[:, None]).all() and (np.abs(sk.sum(axis=1) - smooth['stays']) <= bar).all()
    # abn_hmm_accumulate on the kernel's gamma against the all-float64 restatement: tests/test_gpu_hmm_bw.py's bar
    ref64 = case.reference(stay, True)[0]
    aug = gmm_np.augment(case.xc, case.bad, np.float64)
    allowed_g = np.where(~case.bad[:, None], ref64['post'] * np.expm1(2.0 * case.rows(S))[:, None] + FLOOR, 0.0)
    g = smooth['post'].astype(np.float64)
    bar_sums = (frames_per_range(len(case.x), K, 0) + 2) * U * (g.T @ np.abs(aug)) + allowed_g.T @ np.abs(aug)
    e_sums = np.abs(stats['sums'] - ref64['post'].T @ aug)
    assert np.isfinite(stats['sums']).all() and (e_sums <= bar_sums).all(), (e_sums / np.maximum(bar_sums, 1e-300)).max()
    assert not stats['sums'][dead].any()
    e = hr.sticky_errors(case, stay, smooth['post'], filt['post'], smooth['loglik'], smooth['stays'])
    for k in e:
        note('in range, sticky: %s over its bar' % k, e[k].max())
    live = bar > 0
    note('in range, sticky: stay_k over its bar', (np.abs(sk - ref_sk)[live] / bar[live, None]).max() if live.any() else 0.0)
    note('in range, sticky: accumulate over its bar', (e_sums / np.maximum(bar_sums, 1e-300)).max())
    print('largest figures so far:', WORST)


@pytest.mark.parametrize('c', OUT_STICKY, ids=sticky_id)
def test_sticky_chain_in_the_window_is_run_and_reported(c):
    K, L, gap, i = c
    stay = hr.STAYS[i]
    case = hr.sticky_case(K, L, gap, bad_rows=hr.bad_rows_for(L))
    ref64, ref32 = case.reference(stay, True)
    stats, smooth, filt = sticky_runs(case, stay)
    for got in (smooth, filt):
        assert got['post'].shape == (len(case.x), K) and np.array_equal(got['n_good'], ref64['n_good']) and not got['post'][case.bad].any()
    assert stats['stay_k'].shape == (hr.N_UTT, K) and stats['sums'].shape == (K, 2 * case.D + 1)
    mine = hr.sticky_errors(case, stay, smooth['post'], filt['post'], smooth['loglik'], smooth['stays'])
    theirs = hr.sticky_errors(case, stay, ref32['post'], ref32['ahat'], ref32['loglik'], ref32['stays'])
    with np.errstate(all='ignore'):
        finite = np.isfinite(smooth['post']).all() and np.isfinite(smooth['loglik']).all() and np.isfinite(stats['sums']).all()
        sums_ok = (np.abs(smooth['post'].astype(np.float64).sum(axis=1) - 1.0)[~case.bad] <= hr.row_sum_bar(case)[~case.bad]).all()
    print('%s stay %.7g (with BAD rows): error over the bar, device / float32 restatement: %s; finite %s, post >= 0 %s, row sums %s'
          % (case.tag, stay, ', '.join('%s %.3g / %.3g' % (k, mine[k].max(), theirs[k].max()) for k in mine), finite,
             bool((smooth['post'] >= 0).all()), sums_ok))
    for k in mine:
        note('window, sticky: device %s over its bar' % k, mine[k].max())
        note('window, sticky: float32 restatement %s over its bar' % k, theirs[k].max())
    print('largest figures so far:', WORST)


# ---- the decoders: exact inputs ----------------------------------------------------------------------------------------------
def geometric_tables(init, trans, L=8):
    """(lx, ld, ls) of the geometric law of `trans` at L durations, or None where the model's host checks refuse it: a
    diagonal entry of 1 (a unit that is never left) has no law, and one at the floor gives q[k][L] = floor^(L - 1), below the
    2^-100 a log table is allowed to hold (hmm.duration_tables says so; asserted here)."""
    from abnet3_amd import hmm
    diag = np.diag(trans).astype(np.float64)
    if (diag >= 1).any():
        with pytest.raises(ValueError):
            hmm.geometric_durations(trans, L)
        return None
    q, r = hmm.geometric_durations(trans, L)
    if q.min() < 2.0 ** -100:
        with pytest.raises(ValueError, match='below 2\\^-100'):
            hmm.duration_tables(q, r)
        return None
    return (hmm.switch_log_transitions(init, trans)[1],) + hmm.duration_tables(q, r)


LENGTHS = (1, 2, 24, 127, 129, 140)
EXACT = [(name, K, e) for e in hr.EPS_EXP for name, K in (('cyclic', 4), ('cyclic', 64), ('cyclic', 128), ('blocks', 4), ('blocks', 64),
                                                          ('blocks', 128), ('left_to_right', 65), ('blocks', 65))]


def far_exact_scores(T, K, seed, D=2):
    """test_gpu_hmm_dense_vit.exact_case's recipe with the frames eight times as far out and few distinct offsets: integer
    frames in 8 [-3, 3], A integer in [-2, 2], B = -0.5, c0 in eighths of [-2, 2].  The float32 scores are exact, hundreds
    apart between units that differ -- more than any floor, so the best path goes through the floor -- and EQUAL between the
    units that drew the same row of A and the same offset (25 x 5 combinations for up to 128 units): ties at the floor."""
    rng = np.random.default_rng(seed)
    x = (8 * rng.integers(-3, 4, size=(T, D))).astype(np.float32)
    A = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = (rng.integers(-2, 3, size=K) / 8.0).astype(np.float32)
    x64, A64 = x.astype(np.float64), A.astype(np.float64)
    s64 = x64 @ A64.T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)
    s = s64.astype(np.float32)
    assert np.array_equal(s.astype(np.float64), s64)
    return dict(x=x, A=A, B=B, c0=c0, s=s)


def exact_sparse_case(name, K, e):
    """far_exact_scores under a matrix whose entries are powers of two: 1/2, 1/4, 1 and the floor, so the log tables hold
    -80 ln 2 or -100 ln 2, rounded once by hmm.log_transitions, beside -ln 2 and 0."""
    from abnet3_amd import hmm
    c = far_exact_scores(int(sum(LENGTHS)), K, seed=1000 * K + e)
    init, trans = hr.transitions(name, K, 2.0 ** -e)
    assert (np.frexp(np.concatenate([trans.ravel(), init]).astype(np.float64))[0] == 0.5).all()      # powers of two, every one
    c['li'], c['lt'] = hmm.log_transitions(init, trans)
    c['init'], c['trans'] = init, trans
    return c


@pytest.mark.parametrize('name,K,e', EXACT)
def test_decoders_on_exact_sparse_inputs_equal_their_restatements(name, K, e):
    from abnet3_amd import hmm
    c = exact_sparse_case(name, K, e)
    T = c['x'].shape[0]
    off = np.cumsum(LENGTHS) - np.array(LENGTHS)
    good = np.ones(T, dtype=bool)
    d = [dev(c[k], np.float32) for k in ('x', 'A', 'B', 'c0')]
    shift = dev(np.zeros(c['x'].shape[1]), np.float32)
    assert c['lt'].min() == np.float32(-e * np.log(2.0))

    def same(got, ref, what):
        got = [host(t) for t in got]
        assert np.array_equal(got[0], ref[0]), (what, np.flatnonzero(got[0] != ref[0])[:10])
        assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[3], ref[3]), what
    li, lt = dev(c['li'], np.float32), dev(c['lt'], np.float32)
    ref = dv.viterbi(c['s'], good, off, LENGTHS, c['li'], c['lt'], ids=np.full(T, -1))
    ref_ids = ref[0]
    same(hmm.dense_viterbi(d[0], off, LENGTHS, shift, d[1], d[2], d[3], li, lt), ref, 'abnz_hmm_dense_viterbi')
    same(hmm.dense_viterbi(d[0], off, LENGTHS, shift, d[1], d[2], d[3], li, lt, min_duration=2),
         dd.viterbi(c['s'], good, off, LENGTHS, c['li'], c['lt'], 2, ids=np.full(T, -1)), 'abnw_hmm_dense_viterbi_dur, S = 2')
    n_ties = dv.ties(c['s'], good, off, LENGTHS, c['li'], c['lt'])
    print('%s K %d floor 2^-%d: %d frames of the chosen paths with a tied argmax' % (name, K, e, n_ties))
    floor_steps = sum(int((c['lt'][a[:-1], a[1:]] == c['lt'].min()).sum()) for a in (ref_ids[o:o + n] for o, n in zip(off, LENGTHS)))
    assert K < 64 or (n_ties > 0 and floor_steps > 0), (n_ties, floor_steps)      # (four units tie and switch too rarely to promise it)
    tables = geometric_tables(c['init'], c['trans'])
    if tables is not None:
        lx, ld, ls = tables
        same(hmm.hsmm_viterbi(d[0], off, LENGTHS, shift, d[1], d[2], d[3], li, dev(lx, np.float32), dev(ld, np.float32), dev(ls, np.float32)),
             hs.viterbi(c['s'], good, off, LENGTHS, c['li'], lx, ld, ls, ids=np.full(T, -1)), 'abnu_hmm_hsmm_viterbi, L = 8')
    else:
        assert name in ('left_to_right', 'blocks') and K == 65


@pytest.mark.parametrize('K', [4, 65, 128, 300])
def test_sticky_decoder_on_exact_inputs_with_tiny_and_retired_weights_equals_its_restatement(K):
    from abnet3_amd import hmm
    T = int(sum(LENGTHS))
    off = np.cumsum(LENGTHS) - np.array(LENGTHS)
    c = far_exact_scores(T, K, seed=K)
    k = np.arange(K)
    w = 2.0 ** -(1.0 + k % 5)
    w[1::4] = 2.0 ** -(60.0 + (k[1::4] // 4) % 20)                           # 2^-60 .. 2^-79
    w[3::7] = 0.0
    for stay in (0.0, 0.5):
        lw, ls, lr = hmm.viterbi_tables(w, stay)
        assert np.array_equal(lw, hmm_vit_np.tables(w, stay)[0]) and lr[np.isfinite(lr)].min() <= np.float32(-60 * np.log(2.0))
        got = hmm.viterbi(dev(c['x'], np.float32), off, LENGTHS, dev(np.zeros(2), np.float32), dev(c['A'], np.float32), dev(c['B'], np.float32),
                          dev(c['c0'], np.float32), dev(lw, np.float32), dev(ls, np.float32), dev(lr, np.float32))
        ref = hmm_vit_np.viterbi(c['s'], np.ones(T, dtype=bool), off, LENGTHS, lw, ls, lr, ids=np.full(T, -1))
        got = [host(t) for t in got]
        assert np.array_equal(got[0], ref[0]) and np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
        assert np.array_equal(got[3], ref[3]) and not (w == 0)[got[0]].any()


# ---- the decoders: the float cases, in range or not ------------------------------------------------------------------------------
FLOAT_DECODER_CASES = [(name, K, L, e, gap) for name in hr.MATRICES for K, L in hr.SHAPES for e in hr.EPS_EXP for gap in (60, 300)]


@pytest.mark.parametrize('c', FLOAT_DECODER_CASES, ids=case_id)
def test_dense_decoders_on_the_float_cases_are_within_their_allowance(c):
    from abnet3_amd import hmm
    case = hr.dense_case(*c)
    d, K = case.d, case.K
    s64 = case.scores()['s64']
    scale = gmm_np.score_scale(case.xc, case.bad, case.A, case.B, case.c0)
    E = dv.score_bound(scale, case.D).max(axis=1)
    good = np.ones(c[2], dtype=bool)
    used = 0.0
    for S in (1, 2):
        (ids, lp, nsw, ng), li, lt = decode(case, S)
        lmax = dv.table_max(li, lt)
        assert np.array_equal(ng, case.lens)
        for u, (o, n) in enumerate(zip(case.off, case.lens)):
            sl = slice(o, o + n)
            smax = np.abs(s64[sl]).max() + E[sl].max()
            if S == 1:
                opt, allow, j64 = dv.optimum_f64(s64[sl], good, li, lt), 2.0 * n * dv.delta(E[sl], smax, lmax), dv.J(s64[sl], ids[sl], good, li, lt)
            else:
                opt, allow = dd.optimum_f64(s64[sl], good, li, lt, S), 2.0 * n * dd.delta(E[sl], smax, lmax, S)
                j64 = dd.J_runs(s64[sl], ids[sl], good, li, lt, S)
            assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0) and abs(lp[u] - opt) <= allow, (case.tag, S, u)
            used = max(used, (opt - j64) / allow, abs(lp[u] - opt) / allow)
    tables = geometric_tables(case.init, case.trans)
    assert (tables is None) == (c[0] == 'left_to_right' or (c[0] == 'counts' and K >= 65) or (c[0], K) == ('blocks', 65))
    if tables is not None:
        li = hmm.log_transitions(case.init, case.trans)[0]
        lx, ld, ls = tables
        out = hmm.hsmm_viterbi(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], dev(li, np.float32), dev(lx, np.float32),
                               dev(ld, np.float32), dev(ls, np.float32))
        ids, lp, nsw, ng = (host(t) for t in out)
        lmax = hs.table_max(li, lx, ld, ls)
        for u, (o, n) in enumerate(zip(case.off, case.lens)):
            sl = slice(o, o + n)
            opt = hs.viterbi_one(s64[sl], good, li, lx, ld, ls, np.float64)[1]
            allow = 2.0 * (n + 1) * hs.delta(E[sl], np.abs(s64[sl]).max() + E[sl].max(), lmax, 8)
            j64 = hs.J_runs(s64[sl], ids[sl], good, li, lx, ld, ls)
            assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0) and abs(lp[u] - opt) <= allow, (case.tag, 'hsmm', u)
            used = max(used, (opt - j64) / allow, abs(lp[u] - opt) / allow)
    note('decoders on the float cases: share of the allowance used', used)
    print('%s: the decoders used %.3g of their allowance' % (case.tag, used))


@pytest.mark.parametrize('K,L', hr.SHAPES)
def test_sticky_decoder_on_the_float_cases_is_within_its_allowance(K, L):
    from abnet3_amd import hmm
    used = 0.0
    for gap in (60, 300):
        case = hr.sticky_case(K, L, gap)
        d = case.d
        s64 = case.scores()['s64']
        E = hmm_vit_np.score_bound(gmm_np.score_scale(case.xc, case.bad, case.A, case.B, case.c0), case.D).max(axis=1)
        good = np.ones(L, dtype=bool)
        for stay in hr.STAYS:
            t32 = hmm.viterbi_tables(case.w32, stay)
            out = hmm.viterbi(d['table'], case.off, case.lens, d['shift'], d['A'], d['B'], d['c0'], *[dev(t, np.float32) for t in t32])
            ids, lp, nsw, ng = (host(t) for t in out)
            lmax = hmm_vit_np.table_max(*t32)
            assert np.array_equal(ng, case.lens) and not (case.w32 == 0)[ids].any()
            for u, (o, n) in enumerate(zip(case.off, case.lens)):
                sl = slice(o, o + n)
                opt = hmm_vit_np.optimum_f64(s64[sl], good, *t32)
                allow = 2.0 * n * hmm_vit_np.delta(E[sl], np.abs(s64[sl]).max() + E[sl].max(), lmax)
                j64 = hmm_vit_np.J(s64[sl], ids[sl], good, *t32)
                assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0) and abs(lp[u] - opt) <= allow, (case.tag, stay, u)
                used = max(used, (opt - j64) / allow, abs(lp[u] - opt) / allow)
    note('sticky decoder on the float cases: share of the allowance used', used)
    print('K %d: the sticky decoder used %.3g of its allowance' % (K, used))
