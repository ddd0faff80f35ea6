"""abn_kmeans_viterbi and KMeansQuantizer.segment on the MI355X against tests/units_np.py.

Exact inputs: x and m small integers, shift = 0, b = -|m|^2 / 2 and penalties whose score-unit value p = penalty / 2 is
a multiple of 1/2 -- every fp32 operation of the score GEMM and of the recurrence is then exact, ties are plentiful, and
ids, objective and n_switch must EQUAL the restatement's.  Random float data is compared through the float64 objective
with the allowance units_np's docstring derives (2 n_good delta)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import kmeans_np  # noqa: E402
import units_np  # noqa: E402

pytestmark = pytest.mark.gpu

LENGTHS = (0, 1, 2, 63, 64, 65, 127, 128, 129, 300)
KS, DS = (1, 5, 64, 65, 129, 300), (1, 31, 32, 33, 100)
PENS = (0.0, 1.0, 3.0, 8.0)                  # in units of the distortion: p = 0, 1/2, 3/2, 4 in score units


def dev(a, dt=np.float32):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def host(t):
    return t.detach().cpu().numpy()


exact_case = units_np.exact_case


def layout(lengths, gap=2):
    """Offsets of utterances laid out in the given order with `gap` rows outside every utterance between them."""
    off, o = [], gap
    for n in lengths:
        off.append(o)
        o += n + gap
    return np.array(off, dtype=np.int64), o


def run(x, m, b, off, lens, penalty, ids=None, shift=None):
    from abnet3_amd import kmeans
    D = x.shape[1]
    shift = np.zeros(D, dtype=np.float32) if shift is None else shift
    out = kmeans.viterbi(dev(x), off, lens, dev(shift), dev(m), dev(b), penalty, ids=ids, want_objective=True)
    torch.cuda.synchronize()
    return tuple(host(t) for t in out)


def check_exact(x, m, b, s, off, lens, penalty):
    T = x.shape[0]
    good = np.ones(T, dtype=bool)
    ref = units_np.viterbi(s, good, off, lens, units_np.score_penalty(penalty))
    ids, obj, nsw = run(x, m, b, off, lens, penalty, ids=torch.full((T,), -7, dtype=torch.int32, device='cuda'))
    assert np.array_equal(ids, ref[0]), np.flatnonzero(ids != ref[0])[:10]
    assert np.array_equal(obj, ref[1]) and np.array_equal(nsw, ref[2])
    return ids, obj, nsw


# ---- 1: exact equality -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('K,D', [(K, D) for K in KS for D in DS])
def test_exact_inputs_equal_the_restatement(K, D):
    penalty = PENS[(KS.index(K) + DS.index(D)) % len(PENS)]
    off, T = layout(LENGTHS)
    x, m, b, s = exact_case(T, K, D, seed=100 * K + D)
    ids, obj, nsw = check_exact(x, m, b, s, off, LENGTHS, penalty)
    # the same utterances handed over in another order: the same rows get the same ids
    perm = np.random.default_rng(K + D).permutation(len(LENGTHS))
    ids2, obj2, nsw2 = run(x, m, b, off[perm], np.array(LENGTHS)[perm], penalty,
                           ids=torch.full((T,), -7, dtype=torch.int32, device='cuda'))
    assert np.array_equal(ids2, ids) and np.array_equal(obj2, obj[perm]) and np.array_equal(nsw2, nsw[perm])


@pytest.mark.parametrize('K', [127, 128])
def test_exact_inputs_on_both_sides_of_the_slab_threshold(K):
    """K <= 128 keeps the score slab in LDS, K = 129 (the grid above) is the first with the slab in the workspace."""
    lens = np.array([129, 300, 1, 128])
    off, T = layout(lens)
    x, m, b, s = exact_case(T, K, 33, seed=K)
    check_exact(x, m, b, s, off, lens, 3.0)


def test_exact_inputs_at_the_largest_k():
    from abnet3_amd import kmeans
    K = kmeans.viterbi_max_k()
    x, m, b, s = exact_case(130, K, 8, seed=7)
    check_exact(x, m, b, s, [0], [130], 3.0)


# ---- 2: no penalty = the assign pass -------------------------------------------------------------------------------------
def quantizer(K, D, metric, seed, spread=1.0):
    from abnet3_amd.kmeans import KMeansQuantizer
    rng = np.random.default_rng(seed)
    q = KMeansQuantizer(K, metric=metric)
    c = rng.normal(size=(K, D)) * spread
    if metric == 'cosine':
        c /= np.sqrt((c * c).sum(axis=1, keepdims=True))
    q.centroids_, q.counts_ = c, np.ones(K)
    q.shift_ = np.zeros(D, dtype=np.float32) if metric == 'cosine' else (0.1 * rng.normal(size=D)).astype(np.float32)
    return q, rng


@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
@pytest.mark.parametrize('T,K,D', [(1000, 129, 40), (700, 300, 280)])
def test_zero_penalty_gives_predict_ids(T, K, D, metric):
    q, rng = quantizer(K, D, metric, seed=T + K)
    table = dev(rng.normal(size=(T, D)))
    plain = host(q.predict(table))
    seg = host(q.segment(table, 0.0))
    assert np.array_equal(seg, plain)
    assert q.last_n_switch_.tolist() == [units_np.switches(plain)] and q.last_objective_.shape == (1,)


# ---- 3: BAD frames -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('metric', ['euclidean', 'cosine'])
def test_bad_frames_keep_minus_one_and_the_chain_passes_over_them(metric):
    K, D = 9, 12
    q, rng = quantizer(K, D, metric, seed=21)
    feats = {'u%d' % i: rng.normal(size=(n, D)).astype(np.float32) for i, n in enumerate((140, 5, 260, 3))}
    bad = {'u0': [0, 70, 139], 'u1': [], 'u2': [127, 128, 200], 'u3': [0, 1, 2]}       # first / middle / last; block edges; all
    for k, rows in bad.items():
        for j, r in enumerate(rows):
            feats[k][r] = 0.0 if (metric == 'cosine' and j % 2 == 0) else np.inf
            if j % 2 and metric == 'euclidean':
                feats[k][r, 3] = np.nan
    clean = {k: np.delete(v, bad[k], axis=0) for k, v in feats.items()}
    for penalty in (0.0, 0.5, 4.0):
        ids = q.segment(feats, penalty)
        obj, nsw = q.last_objective_.copy(), q.last_n_switch_.copy()
        ref = q.segment(clean, penalty)
        for k in feats:
            assert (ids[k][bad[k]] == -1).all() and ids[k].shape == (feats[k].shape[0],)
            assert np.array_equal(np.delete(ids[k], bad[k]), ref[k]) and (ref[k] >= 0).all()
        assert np.array_equal(obj, q.last_objective_) and np.array_equal(nsw, q.last_n_switch_)
        assert obj[3] == 0.0 and nsw[3] == 0


# ---- 4: more utterances than workgroups ----------------------------------------------------------------------------------
def test_thousands_of_short_utterances_reuse_the_slabs():
    n = 3000
    x, m, b, s = exact_case(3 * n + 1, 5, 4, seed=4)
    off = 1 + 3 * np.arange(n, dtype=np.int64)
    ids, obj, nsw = check_exact(x, m, b, s, off, np.full(n, 3), 1.0)
    assert ids[0] == -7 and nsw.max() > 0


# ---- 5: reproducible, and nothing outside the utterances is written ------------------------------------------------------
def test_two_calls_are_bit_identical_and_other_rows_are_untouched():
    rng = np.random.default_rng(8)
    lens = rng.integers(1, 400, size=300)
    off, T = layout(lens, gap=3)
    K, D = 200, 40
    x = rng.normal(size=(T, D)).astype(np.float32)
    m, b = kmeans_np.tables(rng.normal(size=(K, D)))
    sentinel = torch.arange(T, dtype=torch.int32, device='cuda') - 100000
    a = run(x, m, b, off, lens, 2.0, ids=sentinel.clone())
    c = run(x, m, b, off, lens, 2.0, ids=sentinel.clone())
    assert all(np.array_equal(u, v) for u, v in zip(a, c)) and a[1].tobytes() == c[1].tobytes()
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    assert np.array_equal(a[0][~inside], host(sentinel)[~inside]) and (~inside).sum() >= 3 * 301
    assert (a[0][inside] >= 0).all() and (a[0][inside] < K).all()


# ---- 6: the penalty's effect -----------------------------------------------------------------------------------------------
def test_switches_fall_with_the_penalty_and_a_huge_one_leaves_one_unit():
    lens = np.array([300, 129, 64, 5, 1])
    off, T = layout(lens)
    x, m, b, s = exact_case(T, 65, 33, seed=12)
    before = None
    for penalty in (0.0, 1.0, 2.0, 5.0, 16.0, 64.0, 1024.0):
        ids, obj, nsw = check_exact(x, m, b, s, off, lens, penalty)
        assert before is None or (nsw <= before).all(), (penalty, nsw, before)
        before = nsw
    huge = 2.0 * 2.0 * 300 * float(np.abs(s).max()) + 2.0          # penalty / 2 above 2 len max|s|
    ids, obj, nsw = check_exact(x, m, b, s, off, lens, huge)
    assert (nsw == 0).all()
    for o, n in zip(off, lens):
        col = s[o:o + n].astype(np.float64).sum(axis=0)
        assert (ids[o:o + n] == int(np.argmax(col))).all() and obj[list(off).index(o)] == col.max()


# ---- 7: random float data against the float64 optimum ----------------------------------------------------------------------
@pytest.mark.parametrize('K', [37, 300])
def test_float_data_is_within_the_derived_allowance_of_the_float64_optimum(K):
    rng = np.random.default_rng(K)
    D = 40
    lens = rng.integers(200, 401, size=12)
    off, T = layout(lens, gap=0)
    centres = rng.normal(size=(K, D))
    lab = np.repeat(rng.integers(0, K, size=T // 7 + 1), 7)[:T]
    x = (centres[lab] + 0.7 * rng.normal(size=(T, D))).astype(np.float32)
    xc, badrow, shift = kmeans_np.prepare(x)
    m, b = kmeans_np.tables(centres - shift.astype(np.float64) + 0.05 * rng.normal(size=(K, D)))
    s64, E = kmeans_np.scores(xc, badrow, m, b)
    assert not badrow.any()
    for penalty in (0.0, 3.0, 20.0, 200.0):
        p = float(units_np.score_penalty(penalty))
        ids, obj, nsw = run(x, m, b, off, lens, penalty, shift=shift)
        for u, (o, n) in enumerate(zip(off, lens)):
            sl = slice(o, o + n)
            opt = units_np.optimum_f64(s64[sl], np.ones(n, dtype=bool), p)
            allow = 2.0 * n * units_np.delta(E[sl], np.abs(s64[sl]).max() + E[sl].max(), p)
            j64 = units_np.J(s64[sl], ids[sl], p)
            print('K %d penalty %g utt %d: optimum %.6f J64(device ids) %.6f device objective %.6f allowance %.3g switches %d'
                  % (K, penalty, u, opt, j64, obj[u], allow, nsw[u]))
            assert opt - allow <= j64 <= opt + 1e-9 * (abs(opt) + 1.0)       # (the upper side: float64 rounding of the two sums only)
            assert abs(obj[u] - opt) <= allow
            assert nsw[u] == units_np.switches(ids[sl])


# ---- 8: the public layer -----------------------------------------------------------------------------------------------------
def test_corpus_through_segment_and_quantize_keeps_names_lengths_and_times():
    from abnet3_amd import kmeans
    from abnet3_amd.dataloader import DeviceCorpus
    from test_gpu_abx import synthetic_set
    items, feats, times = synthetic_set(np.random.default_rng(5), n_items=40, D=13, n_phones=4)
    corpus = DeviceCorpus(feats, times)
    q = kmeans.KMeansQuantizer(8, n_iter=5).fit(corpus)
    plain = q.predict(corpus)
    assert q.last_objective_ is None
    ids = q.segment(corpus, 6.0)
    assert list(ids) == corpus.names and q.last_objective_.shape == (len(corpus.names),)
    assert q.last_n_switch_.dtype == np.int32 and q.last_objective_.dtype == np.float64
    for i, k in enumerate(corpus.names):
        assert ids[k].dtype == np.int32 and ids[k].shape == (corpus.length[k],)
        assert q.last_n_switch_[i] == units_np.switches(ids[k])
    same = q.predict(corpus, penalty=6.0)
    assert all(np.array_equal(same[k], ids[k]) for k in ids)
    assert all(np.array_equal(a, c) for a, c in zip(q.segment(feats, 6.0).values(), ids.values()))
    seq_plain, seq_pen = kmeans.unit_sequences(plain), kmeans.unit_sequences(ids)
    assert all(len(seq_pen[k]) <= len(seq_plain[k]) for k in ids)
    assert sum(len(v) for v in seq_pen.values()) < sum(len(v) for v in seq_plain.values())
    seg = kmeans.segments(ids)
    assert all(np.array_equal(seg[k][2], seq_pen[k]) and int((seg[k][1] - seg[k][0]).sum()) == corpus.length[k] for k in ids)
    quant = q.quantize(corpus, penalty=6.0)
    assert isinstance(quant, DeviceCorpus) and quant.names == corpus.names and quant.total == corpus.total
    flat = np.concatenate([ids[k] for k in corpus.names])
    for k in corpus.names:
        assert quant.length[k] == corpus.length[k] and quant.offset[k] == corpus.offset[k]
        assert np.array_equal(quant.times[k], corpus.times[k])
    assert np.array_equal(host(quant.table), q.centroids_.astype(np.float32)[flat])
    assert torch.equal(q.quantize(corpus).table, q.quantize(corpus, penalty=None).table)
    with pytest.raises(ValueError, match='penalty'):
        q.segment(corpus, -1.0)
    with pytest.raises(ValueError, match='penalty'):
        q.quantize(corpus, penalty=float('nan'))
    with pytest.raises(ValueError, match='D = 5'):
        q.segment(torch.zeros(10, 5, device='cuda'), 1.0)
    with pytest.raises(ValueError, match='outside the table'):
        kmeans.viterbi(corpus.table, [0], [corpus.total + 1], *q.device_tables(corpus.table.device)[:3], 1.0)
    with pytest.raises(ValueError, match='kmeans.viterbi: utterances overlap'):
        kmeans.viterbi(corpus.table, [0, 2], [3, 2], *q.device_tables(corpus.table.device)[:3], 1.0)
