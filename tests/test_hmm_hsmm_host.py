"""Explicit unit durations on the host: the numpy restatement of the semi-Markov decoder (tests/hmm_hsmm_np.py) against brute
force and against the plain full-transition recurrence under geometric durations, the run statistics on hand-made ids, the
duration update against the score it is meant to maximise, the float64 training loop on the planted corpus, the Python
layer's checks and files, and the abnu_ ledger of include/abnet3_hip_next.h.  No kernel runs here."""
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_hard_np as hh  # noqa: E402
import hmm_hsmm_np as hs  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')
NAMES = {'abnu_hmm_hsmm_max_duration', 'abnu_hmm_hsmm_viterbi_ws_bytes', 'abnu_hmm_hsmm_viterbi', 'abnu_hmm_run_stats'}


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def halves(rng, hi, size):
    return (-rng.integers(0, hi, size=size) / 2.0).astype(np.float32)


# ---- the restatement against brute force -------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,L', [(K, L) for K in (1, 2, 3) for L in (2, 3)])
def test_the_restatement_finds_the_brute_force_optimum_and_a_path_that_attains_it(K, L):
    rng = np.random.default_rng(10 * K + L)
    tied = 0
    for n in range(1, 8):
        for trial in range(3):
            s = (rng.integers(-3, 4, size=(n, K)) / 2.0).astype(np.float32)        # coarse values: ties are plentiful
            li, lx, ld, ls = halves(rng, 5, K), halves(rng, 5, (K, K)), halves(rng, 7, (K, L)), halves(rng, 3, K)
            good = np.ones(n, dtype=bool)
            if trial == 2 and n > 1:
                good[rng.integers(0, n, size=2)] = False              # BAD frames, the first or the last among them now and then
            best, arg = hs.brute_force(s, good, li, lx, ld, ls)
            for dtype in (np.float32, np.float64):                     # (halves: every add is exact in both)
                ids, lp, nsw, ng = hs.viterbi_one(s, good, li, lx, ld, ls, dtype)
                assert lp == best and ng == int(good.sum())
                assert tuple(ids[good].tolist()) in arg and (ids[~good] == -1).all()
                assert hs.J_runs(s, ids, good, li, lx, ld, ls) == best
                assert nsw == max(len(hs.runs(ids[good])) - 1, 0)
            tied += len(arg) > 1
    assert K == 1 or tied > 0                                          # ties did occur


def test_an_utterance_without_a_good_frame_and_the_tail_law():
    ld, ls = np.log(np.array([[0.5, 0.25, 0.25]])), np.log(np.array([0.5]))
    assert hs.viterbi_one(np.zeros((3, 1)), np.zeros(3, dtype=bool), [0.0], [[0.0]], ld, ls)[1:] == (0.0, 0, 0)
    assert hs.duration_log_prob(ld, ls, 0, 2) == ld[0, 1] and hs.duration_log_prob(ld, ls, 0, 3) == ld[0, 2]
    assert hs.duration_log_prob(ld, ls, 0, 6) == ld[0, 2] + 3 * ls[0]
    # K = 1: one segment of the whole utterance, whatever its length
    for n in (1, 2, 3, 9):
        ids, lp, nsw, ng = hs.viterbi_one(np.zeros((n, 1)), np.ones(n, dtype=bool), [0.0], [[0.0]], ld, ls, np.float64)
        assert ids.tolist() == [0] * n and nsw == 0 and abs(lp - hs.duration_log_prob(ld, ls, 0, n)) < 1e-12


# ---- geometric durations: the plain model ----------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,L', [(2, 2), (3, 4), (5, 8), (4, 32)])
def test_geometric_durations_give_the_plain_models_optimum(K, L):
    """Under hmm.geometric_durations the semi-Markov score of a path is the plain model's log joint plus log(1 - trans[k][k]) of
    the LAST unit (the semi-Markov score closes the last segment).  So the float64 optimum equals the optimum of
    tests/hmm_dense_vit_np.py's recurrence on the same model with that closing term added to the last good frame's scores; with
    a constant diagonal it is that recurrence's optimum plus the constant."""
    from abnet3_amd import hmm
    rng = np.random.default_rng(K * L)
    for const_diag in (True, False):
        trans = rng.dirichlet(np.full(K, 2.0), size=K)
        diag = np.full(K, 0.7) if const_diag else rng.uniform(0.3, 0.9, size=K)
        trans[np.arange(K), np.arange(K)] = 0.0
        trans = trans / trans.sum(axis=1, keepdims=True) * (1.0 - diag)[:, None] + np.diag(diag)
        init = rng.dirichlet(np.full(K, 2.0))
        q, r = hmm.geometric_durations(trans, L)
        assert np.allclose(q.sum(axis=1), 1.0, atol=1e-12) and np.array_equal(r, np.diag(trans))
        li, lx, ld, ls = hs.log_tables64(init, trans, q, r)
        lt = np.log(trans)
        for n in (1, 2, L, L + 1, 3 * L + 5):
            s = 3.0 * rng.normal(size=(n, K))
            good = rng.random(n) > 0.15
            good[0] |= not good.any()
            ids, lp, nsw, ng = hs.viterbi_one(s, good, li, lx, ld, ls, np.float64)
            closed = s.copy()
            closed[np.flatnonzero(good)[-1]] += np.log1p(-np.diag(trans))
            opt = dv.optimum_f64(closed, good, li, lt)
            assert abs(lp - opt) <= 1e-10 * (abs(opt) + 1.0)
            ref = dv.viterbi_one(closed, good, li, lt, dtype=np.float64)
            assert np.array_equal(ids, ref[0]) and nsw == ref[2] and ng == ref[3]      # (continuous scores: no ties)
            if const_diag:
                assert abs(lp - (dv.optimum_f64(s, good, li, lt) + np.log1p(-0.7))) <= 1e-10 * (abs(opt) + 1.0)
                assert np.array_equal(ids, dv.viterbi_one(s, good, li, lt, dtype=np.float64)[0])


# ---- the run statistics ------------------------------------------------------------------------------------------------------------
def test_run_stats_on_hand_made_ids():
    K, L = 3, 4
    # run lengths L - 1, L and L + 1
    ids = np.array([0] * 3 + [1] * 4 + [2] * 5)
    dur, tail = hs.run_stats(ids, [0], [12], K, L)
    assert dur.tolist() == [[0, 0, 1, 0], [0, 0, 0, 1], [0, 0, 0, 1]] and tail.tolist() == [0, 0, 1]
    # a BAD frame inside a run does not break it, nor does an id >= K; both are passed over
    ids = np.array([1, 1, -1, 1, 7, 1, 1, 0])
    dur, tail = hs.run_stats(ids, [0], [8], K, L)
    assert dur.tolist() == [[1, 0, 0, 0], [0, 0, 0, 1], [0, 0, 0, 0]] and tail.tolist() == [0, 1, 0]
    # two utterances ending and starting on the same unit are two runs; the row between them counts nothing
    ids = np.array([2, 2, 2, 1, 2, 2])
    dur, tail = hs.run_stats(ids, [0, 4], [3, 2], K, L)
    assert dur.tolist() == [[0, 0, 0, 0], [0, 0, 0, 0], [0, 1, 1, 0]] and tail.tolist() == [0, 0, 0]
    # the order of the utterances does not matter; an utterance of BAD frames only adds nothing
    both = hs.run_stats(ids, [4, 0], [2, 3], K, L)
    assert np.array_equal(both[0], dur) and np.array_equal(both[1], tail)
    assert hs.run_stats(np.array([-1, 5, -1]), [0], [3], K, L)[0].sum() == 0
    # the sum over the runs of their frames is the number of good frames
    rng = np.random.default_rng(0)
    ids = rng.integers(-1, K + 1, size=500)
    for L in (2, 5, 32):
        dur, tail = hs.run_stats(ids, [0, 250], [250, 250], K, L)
        assert (dur * np.arange(1, L + 1)).sum() + tail.sum() == int(((ids >= 0) & (ids < K)).sum())


def test_duration_update_maximises_the_duration_part_of_the_path_score():
    from abnet3_amd import hmm
    rng = np.random.default_rng(3)
    K, L = 5, 6
    dur = rng.integers(1, 40, size=(K, L)).astype(np.int64)
    tail = rng.integers(1, 200, size=K).astype(np.int64)
    q0, r0 = hmm.geometric_durations(np.full((K, K), 1.0 / K), L)
    q, r = hmm.duration_update(dur, tail, q0, r0, alpha=0.0)
    assert np.allclose(q.sum(axis=1), 1.0, atol=1e-12) and np.allclose(q, dur / dur.sum(axis=1, keepdims=True), atol=1e-15)
    assert np.allclose(r, tail / (tail + dur[:, -1]), atol=1e-15)
    rq, rr = hs.duration_update(dur, tail, q0, r0, 0.0)
    assert np.allclose(q, rq, atol=1e-15) and np.allclose(r, rr, atol=1e-15)
    best = hs.duration_score(dur, tail, q, r)
    for k in range(K):                                                 # a perturbation of each row, and of each r, scores less
        for trial in range(5):
            q2 = q.copy()
            q2[k] = q2[k] * np.exp(0.2 * rng.normal(size=L))
            q2[k] /= q2[k].sum()
            assert hs.duration_score(dur, tail, q2, r) < best
            r2 = r.copy()
            r2[k] = min(max(r2[k] + 0.05 * rng.choice([-1, 1]) * (1 + trial), 1e-3), 1 - 1e-3)
            assert hs.duration_score(dur, tail, q, r2) < best
    # with a pseudo-count: the formula, the restatement, and the old law where nothing was seen at alpha = 0
    dur[2], tail[2] = 0, 0
    q, r = hmm.duration_update(dur, tail, q0, r0, alpha=0.0)
    assert np.allclose(q[2], q0[2], atol=1e-15) and r[2] == r0[2]
    q, r = hmm.duration_update(dur, tail, q0, r0, alpha=0.5)
    assert np.allclose(q, (dur + 0.5) / (dur.sum(axis=1, keepdims=True) + L * 0.5), atol=1e-15)
    assert np.allclose(r, (tail + 0.5) / (tail + dur[:, -1] + 1.0), atol=1e-15) and np.allclose(q[2], 1.0 / L) and r[2] == 0.5
    rq, rr = hs.duration_update(dur, tail, q0, r0, 0.5)
    assert np.allclose(q, rq, atol=1e-15) and np.allclose(r, rr, atol=1e-15)
    # the floor: nothing below TRANS_MIN, rows still sum to 1, the tables finite
    dur[:] = 0
    dur[:, 0] = 9
    q, r = hmm.duration_update(dur, np.zeros(K), q0, r0, alpha=0.0)
    assert q.min() >= hmm.TRANS_MIN * 0.99 and np.allclose(q.sum(axis=1), 1.0) and (r == r0).all()
    ld, ls = hmm.duration_tables(q, r)
    assert np.isfinite(ld).all() and np.isfinite(ls).all()


# ---- the float64 training loop on the planted corpus -----------------------------------------------------------------------------
def planted_start():
    x, lens, means, z = hs.planted_corpus()
    shift = x.astype(np.float64).mean(axis=0).astype(np.float32)
    m0, v0, t0, i0 = hh.planted_start(means, 0)
    return x, lens, means, z, shift, m0, v0, t0, i0


def test_the_float64_loop_recovers_the_planted_lengths():
    from abnet3_amd import hmm
    x, lens, means, z, shift, m0, v0, t0, i0 = planted_start()
    L = hs.PLANTED_L
    q0, r0 = hmm.geometric_durations(t0, L)
    gv = x.astype(np.float64).var(axis=0)
    lps, m, v, trans, init, q, r, ids = hs.fit_viterbi(hmm, x, lens, shift, m0 - shift.astype(np.float64), v0, gv, t0, i0, q0, r0,
                                                        n_iter=10, tol=-np.inf, alpha=0.0)
    print('viterbi_log_probs %s\nmodes %s, r %s' % (lps, (np.argmax(q, axis=1) + 1).tolist(), r.tolist()))
    assert len(lps) >= 3 and lps[-1] > lps[0] + 0.1
    want = [min(n, L) for n in hs.PLANTED_LENGTHS]
    assert (np.argmax(q, axis=1) + 1).tolist() == want                  # each planted length is the mode; the long unit sits in the tail
    assert (q[np.arange(4), np.array(want) - 1] > 0.9).all()
    long_unit = int(np.argmax(hs.PLANTED_LENGTHS))
    n_long = hs.PLANTED_LENGTHS[long_unit]
    assert abs(r[long_unit] - (n_long - L) / (n_long - L + 1.0)) < 0.02  # the maximum-likelihood tail of runs of 14 at L = 8
    assert (ids == z).mean() > 0.99


# ---- the Python layer --------------------------------------------------------------------------------------------------------------
def test_table_level_calls_and_their_refusals(lib):
    from abnet3_amd import hmm
    assert hmm.hsmm_max_duration() == hmm.HSMM_MAX_DURATION == 32
    trans = np.array([[0.7, 0.2, 0.1], [0.25, 0.5, 0.25], [0.3, 0.3, 0.4]])
    init = np.array([0.2, 0.3, 0.5])
    q, r = hmm.geometric_durations(trans, 5)
    assert q.shape == (3, 5) and q.dtype == np.float64 and np.allclose(q[:, 1], 0.7 ** 0 * np.diag(trans) * (1 - np.diag(trans)))
    assert np.allclose(q[:, 4], np.diag(trans) ** 4)
    ld, ls = hmm.duration_tables(q, r)
    assert ld.dtype == np.float32 and ls.dtype == np.float32 and ld.shape == (3, 5) and ls.shape == (3,)
    assert np.array_equal(ld[:, :4], np.log(q[:, :4]).astype(np.float32)) and np.array_equal(ls, np.log(r).astype(np.float32))
    assert np.array_equal(ld[:, 4], np.log(q[:, 4] * (1 - r)).astype(np.float32))
    li, lx = hmm.switch_log_transitions(init, trans)
    t32 = trans.astype(np.float32).astype(np.float64)
    want = np.log(t32 / (1.0 - np.diag(t32))[:, None])
    off = ~np.eye(3, dtype=bool)
    assert np.array_equal(lx[off], want.astype(np.float32)[off]) and (np.diag(lx) == 0).all() and lx.dtype == np.float32
    assert np.array_equal(li, hmm.log_transitions(init, trans)[0])
    assert np.allclose(np.exp(lx.astype(np.float64))[off].reshape(3, 2).sum(axis=1), 1.0, atol=1e-6)   # where it goes GIVEN that it leaves
    for bad in (1, 33, 2.0, True, None):
        with pytest.raises(ValueError, match='max_duration'):
            hmm.geometric_durations(trans, bad)
    with pytest.raises(ValueError, match='inside'):
        hmm.geometric_durations(np.eye(2), 4)
    with pytest.raises(ValueError, match=r'trans \[K, K\]'):
        hmm.geometric_durations(np.zeros((2, 3)), 4)
    for bq, br, msg in ((q[:, :1], r, 'max_duration'), (np.zeros((3, 33)), r, 'max_duration'), (q, r[:2], 'are needed'),
                        (q * 0.5, r, 'sum to 1'), (np.where(q == q.max(), np.nan, q), r, 'finite'), (q, r * 0.0, '2\\^-100'),
                        (q, np.ones(3), '2\\^-100'), (np.where(np.arange(5) == 0, 0.0, q + q[:, :1] / 4), r, '2\\^-100'),
                        ('x', r, 'are needed')):
        with pytest.raises(ValueError, match=msg):
            hmm.duration_tables(bq, br)
    with pytest.raises(ValueError, match='sum to 1'):
        hmm.switch_log_transitions(init, trans * 0.5)
    # a unit that is (in float32) never left: the off-diagonal sum stands for 1 - trans[j][j], and the tables stay finite
    lx1 = hmm.switch_log_transitions([0.5, 0.5], np.array([[1.0, 2.0 ** -90], [0.5, 0.5]]))[1]
    assert lx1[0, 1] == 0.0 and lx1[1, 0] == 0.0 and np.isfinite(lx1).all()
    assert hmm.switch_log_transitions([1.0], [[1.0]])[1].tolist() == [[0.0]]             # K = 1: nothing to leave for
    dur, tail = np.ones((3, 5)), np.ones(3)
    for kw, msg in ((dict(dur=np.ones((3, 4))), 'dur'), (dict(tail=np.ones(2)), 'dur'), (dict(alpha=-1.0), 'alpha'),
                    (dict(alpha='a'), 'alpha'), (dict(dur=-dur), 'negative'), (dict(tail=np.full(3, np.inf)), 'finite'),
                    (dict(q=q * 0.5), 'sum to 1')):
        args = dict(dur=dur, tail=tail, q=q, r=r, alpha=1e-3)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            hmm.duration_update(**args)
    # hsmm_viterbi and run_stats: the host checks come before anything touches a device
    z = lambda *shape: torch.zeros(shape)
    T, D, K, L = 6, 2, 3, 5
    tabs = dict(table=z(T, D), off=[0], lens=[T], shift=z(D), A=z(K, D), B=z(K, D), c0=z(K), li=z(K), lx=z(K, K), ld=z(K, L), ls=z(K))
    for kw, msg in ((dict(ld=z(K, 1)), 'max_duration'), (dict(ld=z(K, 33)), 'max_duration'), (dict(ld=z(K + 1, L)), 'float32 tensors'),
                    (dict(ls=z(K + 1)), 'float32 tensors'), (dict(lx=z(K, K).double()), 'float32 tensors'), (dict(li=None), 'float32 tensors'),
                    (dict(ld=torch.full((K, L), -np.inf)), 'NaN'), (dict(ls=torch.full((K,), np.nan)), 'NaN'), (dict(off=[0, 3]), 'offsets'),
                    (dict(lens=[T + 1]), 'outside'), (dict(ids=torch.zeros(T)), 'ids')):
        args = dict(tabs)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            hmm.hsmm_viterbi(**args)
    ids = torch.zeros(T, dtype=torch.int32)
    for kw, msg in ((dict(ids=ids.long()), 'ids'), (dict(ids=ids.reshape(2, 3)), 'ids'), (dict(K=0), 'K = '), (dict(K=129), 'K = '),
                    (dict(K=True), 'K = '), (dict(L=1), 'max_duration'), (dict(L=33), 'max_duration'), (dict(lens=[T + 1]), 'outside'),
                    (dict(off=[0, 1], lens=[3, 3]), 'overlap')):
        args = dict(ids=ids, off=[0], lens=[T], K=K, L=L)
        args.update(kw)
        with pytest.raises(ValueError, match=msg):
            hmm.run_stats(**args)


def test_the_model_keeps_checks_and_saves_its_durations(lib, tmp_path):
    from abnet3_amd import hmm
    from test_hmm_host import fitted_mixture
    h = hmm.TransitionHmmPosteriorgram(fitted_mixture(), stay=0.75)
    assert h.dur_ is None and h.dur_tail_ is None
    feats = torch.zeros(5, 2)
    for call in (h.decode, h.quantize):
        with pytest.raises(ValueError, match='no durations'):
            call(feats, durations=True)
    path = str(tmp_path / 'plain.npz')
    h.save(path)
    with np.load(path) as f:
        assert 'dur' not in f.files and 'dur_tail' not in f.files          # a model without durations writes the file it wrote before
    g = hmm.TransitionHmmPosteriorgram.load(path)
    assert g.dur_ is None and g.dur_tail_ is None and np.array_equal(g.trans_, h.trans_)
    for kw in (dict(), dict(q=np.ones((3, 4)) / 4), dict(r=np.full(3, 0.5)), dict(q=np.ones((3, 4)) / 4, r=np.full(3, 0.5), max_duration=4)):
        with pytest.raises(ValueError, match='either'):
            h.set_durations(**kw)
    with pytest.raises(ValueError, match='max_duration'):
        h.set_durations(max_duration=40)
    with pytest.raises(ValueError, match='K = 3'):
        h.set_durations(np.ones((2, 4)) / 4, np.full(2, 0.5))
    with pytest.raises(ValueError, match='sum to 1'):
        h.set_durations(np.ones((3, 4)), np.full(3, 0.5))
    assert h.dur_ is None
    assert h.set_durations(max_duration=6) is h
    q, r = hmm.geometric_durations(h.trans_, 6)
    assert np.array_equal(h.dur_, q) and np.array_equal(h.dur_tail_, r) and h.dur_.dtype == np.float64
    for call in (h.decode, h.quantize):
        with pytest.raises(ValueError, match='min_duration'):
            call(feats, min_duration=2, durations=True)
    q2 = np.full((3, 4), 0.25)
    h.set_durations(q2, np.array([0.5, 0.25, 0.125]))
    assert h.dur_.shape == (3, 4) and h.dur_tail_.tolist() == [0.5, 0.25, 0.125]
    path = str(tmp_path / 'dur.npz')
    h.save(path)
    g = hmm.TransitionHmmPosteriorgram.load(path)
    assert np.array_equal(g.dur_, h.dur_) and np.array_equal(g.dur_tail_, h.dur_tail_) and np.array_equal(g.trans_, h.trans_)
    from abnet3_amd.gmm import GmmPosteriorgram
    assert GmmPosteriorgram.load(path).n_components == 3                     # still the mixture's file
    # training: the letter d is fit_viterbi's alone
    with pytest.raises(ValueError, match='params'):
        h.fit(feats, params='mvtid')
    with pytest.raises(ValueError, match='params'):
        hmm.check_dense_params('x', 'd')
    plain = hmm.TransitionHmmPosteriorgram(fitted_mixture(), stay=0.75)
    with pytest.raises(ValueError, match='max_duration'):
        plain.fit_viterbi(feats, params='mvtid')
    with pytest.raises(ValueError, match='max_duration'):
        plain.fit_viterbi(feats, params='d', max_duration=1)
    with pytest.raises(ValueError, match='min_duration'):
        plain.fit_viterbi(feats, params='mvtid', max_duration=4, min_duration=2)
    for bad in ('dd', 'mvtidx', 'ds'):
        with pytest.raises(ValueError, match='params'):
            plain.fit_viterbi(feats, params=bad, max_duration=4)
    assert plain.dur_ is None and plain.viterbi_log_probs == []
    # the command line
    with pytest.raises(SystemExit):
        hmm.main(['fit-trans', 'a', 'b', 'c', '--viterbi', '--max-duration', 'x'])
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read()
    assert 'abnu_hmm_hsmm_viterbi' in text and '--max-duration' in text and '--durations' in text
    assert 'a duration distribution, a' not in text and 'duration distributions;' not in text
    assert '--hmm-max-duration' in open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()


# ---- the library -------------------------------------------------------------------------------------------------------------------
def test_the_sixth_section_of_the_header_is_the_ledger(lib):
    from abnet3_amd import _lib
    assert set(_lib.NEXT6_SYMBOLS) == NAMES
    others = set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS) | set(_lib.NEXT4_SYMBOLS) | \
        set(_lib.NEXT5_SYMBOLS)
    assert not NAMES & others
    header = open(HEADER).read()
    assert set(re.findall(r'\b(abnu_\w+)\s*\(', header)) >= NAMES
    assert lib.abn_abi_version() == 20 and _lib.ABI_VERSION == 20
    assert lib.abnu_hmm_hsmm_max_duration() == 32


def test_refusals_that_need_no_launch(lib):
    from abnet3_amd import _lib
    E_ARG, E_UNSUPPORTED, E_WORKSPACE = _lib.E_ARG, _lib.E_UNSUPPORTED, _lib.E_WORKSPACE
    assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(3, 100, 5, 4, 1) == -1 and b'L = 1' in lib.abn_last_error()
    assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(3, 100, 5, 4, 33) == -1
    assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(3, 100, 129, 4, 8) == -1 and lib.abnu_hmm_hsmm_viterbi_ws_bytes(0, 100, 5, 4, 8) == -1
    assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(3, (1 << 20) + 1, 5, 4, 8) == -1
    # min(n_utt, 256) regions of 128 x 128 x 4 + max_len (2 K' + 1) bytes rounded up to 256, the same for every L
    for n_utt, max_len, K, kc in ((3, 100, 5, 16), (300, 1000, 17, 32), (1, 7, 64, 64), (2, 129, 65, 128)):
        per = -(-(128 * 128 * 4 + max_len * (2 * kc + 1)) // 256) * 256
        assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(n_utt, max_len, K, 4, 2) == per * min(n_utt, 256)
        assert lib.abnu_hmm_hsmm_viterbi_ws_bytes(n_utt, max_len, K, 4, 32) == per * min(n_utt, 256)
    p = 256                                                                      # a non-null, aligned address that is never read
    ok = dict(x=p, T=10, D=4, off=p, len=p, n_utt=1, shift=p, A=p, B=p, c0=p, li=p, lx=p, K=5, ids=p, lp=0, nsw=0, ng=0, ws=p,
              ws_bytes=1 << 20, stream=0, ld=p, ls=p, L=8)

    def call(**kw):
        a = dict(ok)
        a.update(kw)
        return lib.abnu_hmm_hsmm_viterbi(*[a[k] for k in ok])
    assert call(T=0) == E_ARG and call(n_utt=0) == E_ARG and call(K=0) == E_ARG and call(D=0) == E_ARG
    assert call(K=129) == E_UNSUPPORTED and call(D=100000) == E_UNSUPPORTED
    for name in ('x', 'off', 'len', 'shift', 'A', 'B', 'c0', 'li', 'lx', 'ids', 'ld', 'ls'):
        assert call(**{name: 0}) == E_ARG, name
    assert call(L=1) == E_ARG and call(L=33) == E_ARG and b'abnu_hmm_hsmm_max_duration' in lib.abn_last_error()
    assert call(ws=0) == E_WORKSPACE and call(ws_bytes=100) == E_WORKSPACE and call(ws=p + 4) == E_ARG
    assert call(L=1, ws=0) == E_ARG                                             # L ahead of the workspace
    okr = dict(ids=p, T=10, off=p, len=p, n_utt=1, K=5, L=8, dur=p, tail=p, stream=0)

    def run(**kw):
        a = dict(okr)
        a.update(kw)
        return lib.abnu_hmm_run_stats(*[a[k] for k in okr])
    assert run(T=0) == E_ARG and run(n_utt=0) == E_ARG and run(K=0) == E_ARG and run(K=129) == E_UNSUPPORTED
    for name in ('ids', 'off', 'len', 'dur', 'tail'):
        assert run(**{name: 0}) == E_ARG, name
    assert run(L=1) == E_ARG and run(L=33) == E_ARG
