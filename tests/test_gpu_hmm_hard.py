"""abnv_hmm_hard_stats, hmm.hard_stats and TransitionHmmPosteriorgram.fit_viterbi on the MI355X against
tests/hmm_hard_np.py.

Exact inputs are integer-valued frames in [-8, 8] with an integer shift: every fp32 sum of the emission part is then exact
(|xc| <= 10, xc^2 <= 100, a few thousand frames: far below 2^24), so counts, sums and n_good must EQUAL the restatement's.
Float data is held to the bar hmm_hard_np's docstring derives from the summation structure -- a sequential fp32 sum per
(range, unit), the ranges in float64: 2^-24 x N[k] x the sum of the unit's |terms| per entry of sums, for every n_ranges, so
twice that between two n_ranges; counts is integer arithmetic and exact throughout.  The training loop is checked on the
planted corpus of tests/test_hmm_hard_host.py: monotone up to the decoder's derived slack 2 n_good delta / n_good
(hmm_dense_vit_np.delta, hmm_dense_dur_np.delta), its statistics equal to the restatement's from the device's own ids at
every iteration, and at the end what the float64 loop reaches with room (successor, |diag - 0.8| <= 0.1, means within 0.3)."""
import copy
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import dirty_memory  # noqa: E402
import hmm_dense_dur_np as dd  # noqa: E402
import hmm_dense_vit_np as dv  # noqa: E402
import hmm_hard_np as hh  # noqa: E402
from test_gpu_hmm_vit import dev, host, mixture, recipe, Scores  # noqa: E402
from test_gpu_hmm_dense_vit import random_transitions  # noqa: E402

pytestmark = pytest.mark.gpu

# the ledger of abnet3_amd._lib.NEXT5_SYMBOLS: the entry the dirty-memory test below reaches, and the host query
DIRTY_CASES = ('abnv_hmm_hard_stats',)
QUERIES = ('abnv_hmm_hard_stats_ws_bytes',)

KS = (1, 2, 3, 16, 17, 64, 127, 128)
DS_SS = ((1, 1), (3, 2), (40, 3), (127, 8), (40, 1), (3, 8))          # every D and every S of the list
bits = dirty_memory.bits


def lengths_for(S):
    return [0, 1, 2, S - 1, S, S + 1, 63, 64, 65, 127, 128, 129, 300, 300, 40, 40, 41]


def exact_set(K, D, S, seed):
    """(x, shift, ids, off, lens): the utterance set of the exact tests, offsets in DESCENDING order, two rows between the
    utterances (the last two touch), every row of the table -- the rows outside the utterances too -- with an id."""
    rng = np.random.default_rng(seed)
    lens = lengths_for(S)
    off, o = [], 2
    for i, n in enumerate(lens):
        off.append(o)
        o += n + (0 if i == len(lens) - 2 else 2)
    T = o
    ids = rng.integers(0, K, size=T).astype(np.int32)                      # random ids, in the gaps as well
    span = lambda i: slice(off[i], off[i] + lens[i])
    last = K - 1
    ids[span(11)] = last                                                   # 129: one unit throughout
    ids[span(10)] = np.where(np.arange(128) % 2 == 0, 0, min(1, last))     # 128: strict alternation
    runs, k, left = [], 0, 127                                             # 127: runs of exactly S and S + 1
    while left > 0:
        n = min(S + (len(runs) & 1), left)
        runs += [k % K] * n
        k, left = k + 1, left - n
    ids[span(9)] = np.array(runs[:127], dtype=np.int32)
    a = ids[span(13)]                                                      # 300: BAD at the start, at the end, inside a run
    a[:3], a[-2:] = -1, -1
    a[100:125] = last
    a[105], a[110], a[111], a[112] = -1, K, -5, K + 1000                   # (the run continues over all four)
    ids[span(14)] = -1                                                     # a whole BAD utterance
    ids[off[15] + lens[15] - 1] = ids[off[16]] = ids[off[16] + 1] = 0      # the same unit on both sides of a boundary
    x = rng.integers(-8, 9, size=(T, D)).astype(np.float32)
    shift = rng.integers(-2, 3, size=D).astype(np.float32)
    for t in rng.integers(0, T, size=6):                                   # a non-finite entry contributes 0, never NaN
        x[t, rng.integers(0, D)] = (np.nan, np.inf, -np.inf)[int(t) % 3]
    x[off[11] + 5, 0] = 3e38                                               # finite, its square is not
    return x, shift, ids, np.array(off[::-1], dtype=np.int64), np.array(lens[::-1], dtype=np.int64)


def run(x, shift, ids, off, lens, K, S=1, n_ranges=0):
    from abnet3_amd import hmm
    out = hmm.hard_stats(dev(x), off, lens, dev(shift), dev(ids, np.int32), K, min_duration=S, n_ranges=n_ranges)
    torch.cuda.synchronize()
    assert out[0].dtype == torch.int64 and out[1].dtype == torch.float64 and out[2].dtype == torch.int32
    assert out[0].shape == (K + 1, K) and out[1].shape == (K, 2 * x.shape[1] + 1) and out[2].shape == (len(off),)
    return tuple(host(t) for t in out)


def raw(x, shift, ids, off, lens, K, S, n_ranges=0):
    """(counts, sums, n_good) host arrays of abnv_hmm_hard_stats with every output and the workspace from torch.empty."""
    from abnet3_amd import _lib
    lib, p = _lib.load(), _lib.ptr
    T, D = x.shape
    n = len(off)
    d = [dev(x), dev(off, np.int64), dev(lens, np.int32), dev(shift), dev(ids, np.int32)]
    counts = torch.empty((K + 1, K), dtype=torch.int64, device='cuda')
    sums = torch.empty((K, 2 * D + 1), dtype=torch.float64, device='cuda')
    ng = torch.empty(n, dtype=torch.int32, device='cuda')
    need = lib.abnv_hmm_hard_stats_ws_bytes(T, n, K, D, n_ranges)
    assert need > 0
    ws = torch.empty(need, dtype=torch.uint8, device='cuda')
    rc = lib.abnv_hmm_hard_stats(p(d[0]), T, D, p(d[1]), p(d[2]), n, p(d[3]), p(d[4]), K, S, n_ranges, p(counts), p(sums), p(ng),
                                 p(ws), need, _lib.stream())
    assert rc == 0, lib.abn_last_error()
    torch.cuda.synchronize()
    return host(counts), host(sums), host(ng)


def same(a, b):
    return all(np.array_equal(bits(u), bits(v)) for u, v in zip(a, b))


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,D,S', [(K, D, S) for K in KS for D, S in DS_SS])
def test_exact_inputs_equal_the_restatement(K, D, S):
    x, shift, ids, off, lens = exact_set(K, D, S, seed=1000 * K + 10 * D + S)
    assert (np.diff(off) < 0).all()
    ref = hh.hard_stats(x, off, lens, shift, ids, K, S)
    got = run(x, shift, ids, off, lens, K, S)
    assert np.array_equal(got[0], ref[0]), np.argwhere(got[0] != ref[0])[:10]
    assert np.array_equal(got[2], ref[2])
    assert np.array_equal(got[1], ref[1]), np.argwhere(got[1] != ref[1])[:10]
    assert np.isfinite(got[1]).all() and got[1][:, -1].sum() == ref[2].sum() < 65536
    # what the set was built to hold
    assert ref[2][::-1][14] == 0 and ref[2][::-1][13] == 300 - 3 - 2 - 4 and ref[0][K, 0] >= 1
    assert ref[0][K].sum() == sum(1 for n in ref[2] if n > 0)
    assert ref[0][K - 1, K - 1] >= max(129 - S, 0) + max(21 - S, 0)              # one unit throughout; the run over the four BAD ids
    # the same utterances in ascending order, and through other ranges: the same counts, the same (exact) sums
    for n_ranges in (1, 3):
        again = run(x, shift, ids, off[::-1].copy(), lens[::-1].copy(), K, S, n_ranges=n_ranges)
        assert np.array_equal(again[0], ref[0]) and np.array_equal(again[1], ref[1]) and np.array_equal(again[2], ref[2][::-1])


def test_more_utterances_than_waves_and_refused_utterances():
    K, D, S = 5, 4, 2
    rng = np.random.default_rng(3)
    n = 3000                                                                  # more than 256 workgroups x 4 waves
    lens = rng.integers(0, 6, size=n)
    off = 1 + 6 * np.arange(n, dtype=np.int64)
    T = 6 * n + 1
    x = rng.integers(-8, 9, size=(T, D)).astype(np.float32)
    ids = rng.integers(-1, K, size=T).astype(np.int32)
    shift = np.zeros(D, dtype=np.float32)
    ref = hh.hard_stats(x, off, lens, shift, ids, K, S)
    assert same(run(x, shift, ids, off, lens, K, S), ref)
    # refused utterances get n_good -1 and add nothing; their neighbours are unaffected
    off2 = np.array([0, -1, 10, T - 3, 30], dtype=np.int64)
    len2 = np.array([5, 4, -2, 4, 300], dtype=np.int32)
    got = raw(x, shift, ids, off2, len2, K, S)
    ref2 = hh.hard_stats(x, [0, 30], [5, 300], shift, ids, K, S)
    assert got[2].tolist() == [ref2[2][0], -1, -1, -1, ref2[2][1]]
    assert np.array_equal(got[0], ref2[0]) and np.array_equal(got[1], ref2[1])


# ---- 2: the decoder's own paths ------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def float_corpus():
    K, D = 8, 13
    rng = np.random.default_rng(11)
    lens = rng.integers(30, 200, size=9)
    x, shift, w, m, v = recipe(K, D, lens, seed=77, run_len=6)
    off = np.cumsum(lens) - lens
    x[off[2] + 4, 1] = np.nan
    x[off[5]:off[5] + 3] = np.inf
    return K, D, lens, off, x, shift, w, m, v


@pytest.mark.parametrize('S', [1, 3])
def test_statistics_of_the_decoders_own_paths(float_corpus, S):
    from abnet3_amd import hmm
    K, D, lens, off, x, shift, w, m, v = float_corpus
    init, trans = random_transitions(K, 5, 0.8)
    h = hmm.TransitionHmmPosteriorgram(mixture(shift, w, m, v), trans, init)
    names = ['u%02d' % i for i in range(len(lens))]
    feats = {k: x[o:o + n] for k, o, n in zip(names, off, lens)}
    dec = h.decode(feats, min_duration=S)
    ids = np.concatenate([dec[k] for k in names])
    counts, sums, ng = run(x, shift, ids, off, lens, K, S)
    assert np.array_equal(ng, h.last_n_good_) and h.n_bad_ == 4 and (ids == -1).sum() == 4
    assert counts[:K].sum() - np.trace(counts[:K]) == h.last_n_switch_.sum() > 0
    assert counts[K].sum() == (h.last_n_good_ > 0).sum() == len(lens)
    assert sums[:, -1].sum() == h.last_n_good_.sum()
    if S == 1:
        assert np.array_equal(counts[:K], hmm.bigram_counts(dec, K))
    else:
        stays = sum(max(n - S, 0) for k in names for _, n in dd.runs(dec[k][dec[k] >= 0]))
        assert np.trace(counts[:K]) == stays > 0
    ref = hh.hard_stats(x, off, lens, shift, ids, K, S, with_abs=True)
    assert np.array_equal(counts, ref[0]) and (np.abs(sums - ref[1]) <= hh.sums_bar(ref[3])).all()


# ---- 3: float data -----------------------------------------------------------------------------------------------------------
@pytest.fixture(scope='module')
def float_case():
    K, D, T = 37, 40, 9000                                                       # 71 blocks of 128 rows: every n_ranges below is real
    rng = np.random.default_rng(5)
    x = (rng.normal(size=(T, D)) * 3.0 + 1.0).astype(np.float32)
    shift = x.mean(axis=0).astype(np.float32)
    ids = rng.integers(-1, K + 1, size=T).astype(np.int32)                       # -1 and K are BAD
    lens = np.array([4000, 1, 2500, 800], dtype=np.int64)                        # rows [5000, 9000), [4500], [1000, 3500), [3600, 4400)
    off = np.array([5000, 4500, 1000, 3600], dtype=np.int64)
    ref = hh.hard_stats(x, off, lens, shift, ids, K, 2, with_abs=True)
    return K, x, shift, ids, off, lens, ref


@pytest.mark.parametrize('n_ranges', [0, 1, 2, 7])
def test_float_data_is_within_the_bar_of_the_summation_structure(float_case, n_ranges):
    K, x, shift, ids, off, lens, ref = float_case
    counts, sums, ng = run(x, shift, ids, off, lens, K, 2, n_ranges=n_ranges)
    bar = hh.sums_bar(ref[3])
    err = np.abs(sums - ref[1])
    print('n_ranges %d: the largest share of the bar used %.3g (largest error %.3g)' % (n_ranges, (err / np.maximum(bar, 1e-300))[:, :-1].max(),
                                                                                          err.max()))
    assert np.array_equal(counts, ref[0]) and np.array_equal(ng, ref[2])
    assert (err <= bar).all() and np.array_equal(sums[:, -1], ref[1][:, -1])


# ---- 4: reproducibility and dirty memory ---------------------------------------------------------------------------------------
def test_two_calls_give_the_same_bits_and_n_ranges_moves_only_the_float_sums(float_case):
    K, x, shift, ids, off, lens, ref = float_case
    outs = {}
    for n_ranges in (1, 2, 7, 0):
        a = run(x, shift, ids, off, lens, K, 2, n_ranges=n_ranges)
        b = run(x, shift, ids, off, lens, K, 2, n_ranges=n_ranges)
        assert same(a, b)
        outs[n_ranges] = a
    bar = hh.sums_bar(ref[3])
    for n_ranges in (2, 7, 0):
        assert np.array_equal(outs[n_ranges][0], outs[1][0]) and np.array_equal(outs[n_ranges][2], outs[1][2])
        assert (np.abs(outs[n_ranges][1] - outs[1][1]) <= 2.0 * bar).all()
    assert not np.array_equal(bits(outs[1][1]), bits(outs[7][1]))                # (the ranges do change the fp32 order)
    perm = np.array([2, 0, 3, 1])                                                # the order of the utterances moves nothing but n_good
    p = run(x, shift, ids, off[perm], lens[perm], K, 2, n_ranges=7)
    assert np.array_equal(p[0], outs[7][0]) and np.array_equal(bits(p[1]), bits(outs[7][1])) and np.array_equal(p[2], outs[7][2][perm])


def test_every_next5_symbol_is_a_dirty_memory_case_or_a_query():
    from abnet3_amd import _lib
    assert set(DIRTY_CASES) | set(QUERIES) == set(_lib.NEXT5_SYMBOLS) and not set(DIRTY_CASES) & set(QUERIES)
    assert not set(_lib.NEXT5_SYMBOLS) & (set(_lib.SYMBOLS) | set(_lib.NEXT_SYMBOLS) | set(_lib.NEXT2_SYMBOLS) | set(_lib.NEXT3_SYMBOLS) |
                                          set(_lib.NEXT4_SYMBOLS))


@pytest.mark.parametrize('K', [5, 65])
def test_outputs_and_workspace_from_dirty_memory_give_the_same_bits(K):
    """The entry of DIRTY_CASES with counts, sums, n_good and the workspace from torch.empty under the three patterns: the same
    bits, and they are the restatement's."""
    from abnet3_amd import _lib
    S, D = 3, 40
    x, shift, ids, off, lens = exact_set(K, D, S, seed=K)
    outs = {}
    with dirty_memory.recorded(_lib.load()) as old_calls:
        for byte in dirty_memory.PATTERNS:
            with dirty_memory.dirty(byte) as count:
                outs[byte] = raw(x, shift, ids, off, lens, K, S)
            assert int(count) >= 4 and count.nbytes > x.shape[0] * 4               # three outputs and the workspace
    assert set(old_calls) <= {'abn_last_error'}
    for byte in dirty_memory.PATTERNS[1:]:
        assert same(outs[byte], outs[0x00]), hex(byte)
    assert same(outs[0xFF], hh.hard_stats(x, off, lens, shift, ids, K, S))


# ---- 5: the training loop ----------------------------------------------------------------------------------------------------
def planted_model(seed=0):
    from abnet3_amd import hmm
    x, lens, means, trans, _ = hh.planted_corpus(seed)
    shift = np.nanmean(x, axis=0).astype(np.float32)
    m0, v0, t0, i0 = hh.planted_start(means, seed)
    g = mixture(shift, np.full(4, 0.25), m0 - shift.astype(np.float64), v0)
    g.gv_ = np.nanvar(x.astype(np.float64), axis=0)
    names = ['u%02d' % i for i in range(len(lens))]
    off = np.cumsum(lens) - lens
    feats = {k: x[o:o + n] for k, o, n in zip(names, off, lens)}
    return hmm.TransitionHmmPosteriorgram(g, t0, i0, alpha=0.0), feats, names, x, lens, off, shift, means


def slack_of(h, x, shift, S):
    """The decoder's per-frame slack under h's parameters: delta of the restatement that decodes at this S."""
    from abnet3_amd import hmm
    g = h.gmm
    sc = Scores(x, shift, np.full(4, 0.25), g.means_ - shift.astype(np.float64), g.variances_)
    good = ~sc.bad
    li, lt = hmm.log_transitions(h.init_, h.trans_)
    E, smax, lmax = sc.E[good].max(), np.abs(sc.s64[good]).max() + sc.E[good].max(), dv.table_max(li, lt)
    return dv.delta(E, smax, lmax) if S == 1 else dd.delta(E, smax, lmax, S)


@pytest.mark.parametrize('S', [1, 3])
def test_fit_viterbi_on_the_planted_corpus(S):
    from abnet3_amd import hmm
    h, feats, names, x, lens, off, shift, means = planted_model()
    whole = copy.deepcopy(h).fit_viterbi(feats, n_iter=10, tol=-np.inf, min_duration=S)
    lps, slacks = [], [slack_of(h, x, shift, S)]
    table, shift_d = dev(x), dev(shift)
    for it in range(len(whole.viterbi_log_probs)):
        # the iteration by hand: the device's own ids under the current parameters, their statistics, the two host updates
        dec = h.decode(feats, min_duration=S)
        ids = np.concatenate([dec[k] for k in names])
        lps.append(float(h.last_log_prob_.sum()) / int(h.last_n_good_.sum()))
        counts, sums, ng = (host(t) for t in hmm.hard_stats(table, off, lens, shift_d, dev(ids, np.int32), 4, min_duration=S))
        ref = hh.hard_stats(x, off, lens, shift, ids, 4, S, with_abs=True)
        assert np.array_equal(counts, ref[0]) and np.array_equal(ng, ref[2]) and np.array_equal(ng, h.last_n_good_)
        assert (np.abs(sums - ref[1]) <= hh.sums_bar(ref[3])).all()
        g = h.gmm
        _, m, v, _, _ = hmm.baum_welch_update(sums, np.zeros(4), 0, g.means_ - shift.astype(np.float64), g.variances_, g.gv_, g.var_floor,
                                              g.min_count, 'mv', weights=np.full(4, 0.25), stay=0.0)
        t, i = hmm.transition_update(counts.astype(np.float64), h.trans_, h.init_, 0.0, 'ti')
        assert (v > 1.5 * g.var_floor * g.gv_).all()                               # the floor does not bind: the M-step is the maximiser
        h.fit_viterbi(feats, n_iter=1, min_duration=S)                           # the same iteration through the loop
        assert len(h.viterbi_log_probs) == 1 and abs(h.viterbi_log_probs[0] - lps[-1]) <= 1e-12 * abs(lps[-1])      # (two float64 sums of 12)
        lps[-1] = h.viterbi_log_probs[0]
        assert np.array_equal(h.trans_, t) and np.array_equal(h.init_, i)
        assert np.array_equal(h.gmm.means_, m + shift.astype(np.float64)) and np.array_equal(h.gmm.variances_, v)
        assert h.n_bad_ == int(np.isnan(x).any(axis=1).sum()) and h.n_starved_ == 0
        slacks.append(slack_of(h, x, shift, S))
    assert np.array_equal(bits(np.array(whole.viterbi_log_probs)), bits(np.array(lps)))       # ten iterations in one call are these
    steps = np.diff(lps)
    allow = np.array([slacks[i] + slacks[i + 1] for i in range(len(steps))])     # 2 n_good delta / n_good, delta of either side
    print('S %d: viterbi_log_probs %s\n  steps %s\n  slack %s, ids changed in the last iteration %d'
          % (S, lps, steps.tolist(), allow.tolist(), whole.last_n_changed_))
    assert len(lps) >= 3 and (steps >= -allow).all() and lps[-1] > lps[0] + 0.1
    assert whole.last_n_changed_ < sum(lens) and whole.n_starved_ == 0
    off_diag = np.where(np.eye(4, dtype=bool), -1.0, whole.trans_)
    assert [int(np.argmax(off_diag[k])) for k in range(4)] == [1, 2, 3, 0]      # the planted successor
    if S == 1:
        assert np.abs(np.diag(whole.trans_) - 0.8).max() <= 0.1 and np.abs(whole.gmm.means_ - means).max() <= 0.3


def test_fit_viterbi_stops_when_no_id_changes_and_leaves_the_mixture_it_came_from():
    h, feats, names, x, lens, off, shift, means = planted_model()
    g0 = h.gmm
    m0 = g0.means_.copy()
    h.fit_viterbi(feats, n_iter=50, tol=-np.inf)
    assert h.last_n_changed_ == 0 and 2 <= len(h.viterbi_log_probs) < 50
    assert h.gmm is not g0 and np.array_equal(g0.means_, m0) and not np.array_equal(h.gmm.means_, m0)
    h2 = planted_model()[0].fit_viterbi(feats, n_iter=50, tol=1e9)               # the gain is below tol at once
    assert len(h2.viterbi_log_probs) == 2


def test_one_transition_iteration_is_the_bigram_update_by_hand():
    from abnet3_amd import hmm
    K, a = 4, 0.5
    h, feats, names, x, lens, off, shift, means = planted_model(1)
    h.alpha = a
    dec = h.decode(feats)
    stats = np.zeros((K + 1, K))
    stats[:K] = hmm.bigram_counts(dec, K)
    for k in names:
        good = dec[k][dec[k] >= 0]
        if len(good):
            stats[K, good[0]] += 1
    t, i = hmm.transition_update(stats, h.trans_, h.init_, a)
    g0 = h.gmm
    h.fit_viterbi(feats, n_iter=1, params='ti')
    assert np.array_equal(h.trans_, t) and np.array_equal(h.init_, i) and len(h.viterbi_log_probs) == 1
    assert np.array_equal(h.gmm.means_, g0.means_) and np.array_equal(h.gmm.variances_, g0.variances_)
    assert h.last_n_changed_ == sum(lens)


def test_the_command_line_trains_and_saves(tmp_path, capsys):
    from abnet3_amd import hmm
    h, feats, names, x, lens, off, shift, means = planted_model()
    gpath, fpath, out = (str(tmp_path / n) for n in ('g.npz', 'f.npz', 'm.npz'))
    h.gmm.weights_ = np.full(4, 0.25)
    h.gmm.save(gpath)
    np.savez(fpath, **feats)
    assert hmm.main(['fit-trans', gpath, fpath, out, '--viterbi', '--min-duration', '2', '--n-iter', '4', '--alpha', '0']) == 0
    line = capsys.readouterr().out
    assert 'Viterbi training' in line and 'min duration 2' in line
    m = hmm.TransitionHmmPosteriorgram.load(out)
    assert 2 <= len(m.viterbi_log_probs) <= 4 and m.log_likelihoods == [] and m.viterbi_log_probs[-1] > m.viterbi_log_probs[0]
    with pytest.raises(ValueError, match='--viterbi'):
        hmm.main(['fit-trans', gpath, fpath, out, '--min-duration', '2'])
    assert hmm.main(['fit-trans', gpath, fpath, out, '--n-iter', '2']) == 0      # without --viterbi: Baum-Welch as before
    assert 'mean log-likelihood' in capsys.readouterr().out
    assert hmm.TransitionHmmPosteriorgram.load(out).viterbi_log_probs == []
