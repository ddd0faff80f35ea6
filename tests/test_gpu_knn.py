"""abn_knn_topk / abn_segment_vectors / KnnPairMiner on the MI355X against the brute-force float64 restatement
(tests/knn_np.py).

The bound: an fp32 dot product of d terms of unit vectors is within delta = 2 (d + 4) 2^-24 of the exact one whatever
the order of summation (knn_np.delta).  knn_np.check_topk asserts, on the float64 side and before it looks at the
kernel's lists, that at least 90 % of a case's queries have no other candidate within delta of their k-th best; on
those the returned set must be the float64 set exactly.  With n candidates spread over a similarity range of width w
about 2 delta n / w of the queries have such a neighbour, so the inputs are dense d-dimensional unit vectors of
intrinsic dimension 6 (similarities spread over (-1, 1)) and d = 1024 (delta = 1.2e-4) is paired with at most 257
candidates, d = 400 with k = 32 likewise."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import knn_np  # noqa: E402

pytestmark = pytest.mark.gpu

EDGES = [1, 31, 32, 33, 255, 256, 257, 1000]
DK = [(4, 1), (40, 10), (400, 32), (1024, 10), (4, 32), (40, 1), (400, 10), (1024, 1), (4, 10), (40, 32), (400, 1),
      (1024, 32)]


def shape_cases():
    cases, n = [], 0
    for nq in EDGES:
        for nc in EDGES:
            d, k = DK[n % len(DK)]
            n += 1
            if nc > 257 and d == 1024:
                d = 400
            if nc > 257 and d == 400 and k == 32:
                k = 10
            cases.append((nq, nc, d, k, n % 2 == 0))
    cases += [(257, 257, 1024, 32, True), (1000, 256, 1024, 32, False), (33, 255, 400, 32, True), (1000, 1000, 40, 32, True)]
    return cases


def unit_rows(rng, n, d, m=6):
    """Dense unit vectors of intrinsic dimension min(m, d): similarities spread over (-1, 1)."""
    m = min(m, d)
    basis = np.linalg.qr(rng.standard_normal((d, m)))[0]
    x = rng.standard_normal((n, m)) @ basis.T
    return (x / np.sqrt((x * x).sum(1))[:, None]).astype(np.float32), basis


def random_meta(rng, n):
    b = rng.integers(0, 200, n)
    return np.stack([rng.integers(0, 4, n), b, b + rng.choice([40, 60], n)], axis=1).astype(np.int32)


def gpu_topk(Q, C, k, qm=None, cm=None):
    from abnet3_amd.discovery import knn_topk
    dev = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).cuda()
    idx, sim = knn_topk(dev(Q), dev(C), k, dev(qm), dev(cm))
    torch.cuda.synchronize()
    return idx.cpu().numpy(), sim.cpu().numpy()


@pytest.mark.parametrize('nq,nc,d,k,meta', shape_cases())
def test_shapes_around_the_tile_edges(nq, nc, d, k, meta):
    rng = np.random.default_rng(nq * 1009 + nc * 13 + d + k)
    C, basis = unit_rows(rng, nc, d)
    x = rng.standard_normal((nq, basis.shape[1])) @ basis.T
    Q = (x / np.sqrt((x * x).sum(1))[:, None]).astype(np.float32)
    qm, cm = (random_meta(rng, nq), random_meta(rng, nc)) if meta else (None, None)
    S = Q.astype(np.float64) @ C.astype(np.float64).T
    excl = knn_np.excluded(qm, cm) if meta else None
    idx, sim = gpu_topk(Q, C, k, qm, cm)
    knn_np.check_topk(idx, sim, S, k, excl, knn_np.delta(d))


def random_walk_files(rng, n_files=24, D=40):
    return [np.cumsum(rng.standard_normal((int(rng.integers(200, 401)), D)), axis=0).astype(np.float32)
            for _ in range(n_files)]


def test_random_walk_corpus_self_search():
    """The issue's case: 24 random-walk files of 200-400 frames, D = 40, lengths (40, 60), shift 5, K = 10, k = 10:
    the table against itself with the overlap exclusion; and abn_segment_vectors on the way."""
    from abnet3_amd.discovery import segment_vectors
    rng = np.random.default_rng(0)
    feats = random_walk_files(rng)
    segs = knn_np.segments([len(f) for f in feats], (40, 60), 5)
    off = np.concatenate(([0], np.cumsum([len(f) for f in feats])))
    row0 = np.array([off[f] + s for f, s, L in segs], dtype=np.int64)
    L = np.array([L for _, _, L in segs], dtype=np.int32)
    table = torch.from_numpy(np.concatenate(feats)).cuda()
    vec, keep = segment_vectors(table, row0, L, 10)
    assert bool(keep.all())
    g = knn_np.gather(feats, segs, 10)
    u64, _ = knn_np.unit64(g)
    v = vec.cpu().numpy()
    assert v.shape == (len(segs), 400)
    assert np.abs(np.sqrt((v.astype(np.float64) ** 2).sum(1)) - 1.0).max() <= 1e-6
    # one rounding of the scale and one of the product: 2^-23 relative, plus a denormal's worth
    assert (np.abs(v - u64) <= 1.001 * 2.0 ** -23 * np.abs(u64) + 1e-30).all()
    meta = np.array([(f, s, s + ln) for f, s, ln in segs], dtype=np.int32)
    S = u64 @ u64.T
    idx, sim = gpu_topk(v, v, 10, meta, meta)
    n_exact = knn_np.check_topk(idx, sim, S, 10, knn_np.excluded(meta, meta), knn_np.delta(400))
    print('%d segments, %d of them free of near ties' % (len(segs), n_exact))
    assert (idx != np.arange(len(segs))[:, None]).all()


def test_segment_vectors_bit_equal_gather():
    """Entries +-1 with K D = 1024: the norm is 32 exactly, so the vector is the gathered frames / 32 bit for bit --
    which pins the frame indices t_j = s + ((2j + 1) L) // (2K); an all-zero segment is flagged."""
    from abnet3_amd.discovery import segment_vectors
    rng = np.random.default_rng(1)
    feats = [rng.choice([-1.0, 1.0], (int(n), 64)).astype(np.float32) for n in (90, 17, 200, 64)]
    feats.append(np.zeros((50, 64), dtype=np.float32))
    segs = knn_np.segments([len(f) for f in feats], (16, 17, 40, 63), 3)
    off = np.concatenate(([0], np.cumsum([len(f) for f in feats])))
    row0 = np.array([off[f] + s for f, s, L in segs], dtype=np.int64)
    L = np.array([L for _, _, L in segs], dtype=np.int32)
    vec, keep = segment_vectors(torch.from_numpy(np.concatenate(feats)).cuda(), row0, L, 16)
    g = knn_np.gather(feats, segs, 16)
    zero = np.array([f == 4 for f, _, _ in segs])
    assert np.array_equal(keep.cpu().numpy(), ~zero) and zero.any()
    assert np.array_equal(vec.cpu().numpy()[~zero], g[~zero] / np.float32(32.0))
    assert not vec.cpu().numpy()[zero].any()
    with pytest.raises(ValueError):
        segment_vectors(torch.zeros(10, 4, device='cuda'), np.array([8]), np.array([3]), 2)


def tie_case(rng, nq, nc, d=16):
    """Small-integer rows, many of them duplicated: every similarity is an integer, exact in fp32 in any order
    (delta = 0 for this case), and equal bit for bit between duplicates: (sim descending, j ascending) determines
    the whole output."""
    C = rng.integers(-2, 3, (nc, d)).astype(np.float32)
    C[1::3] = C[0:nc - 1:3][:len(C[1::3])]
    C[rng.permutation(nc)[:nc // 4]] = C[0]
    Q = rng.integers(-2, 3, (nq, d)).astype(np.float32)
    return Q, C


@pytest.mark.parametrize('k', [1, 10, 32])
def test_exact_ties_go_to_the_smaller_index(k):
    rng = np.random.default_rng(40 + k)
    Q, C = tie_case(rng, 200, 700)
    qm, cm = random_meta(rng, 200), random_meta(rng, 700)
    S = Q.astype(np.float64) @ C.astype(np.float64).T
    for meta in (False, True):
        excl = knn_np.excluded(qm, cm) if meta else None
        ref_idx, ref_sim = knn_np.topk(S, k, excl)
        idx, sim = gpu_topk(Q, C, k, qm if meta else None, cm if meta else None)
        assert np.array_equal(idx, ref_idx)
        assert np.array_equal(sim, ref_sim.astype(np.float32))


@pytest.mark.parametrize('case', ['ties', 'unit'])
def test_split_factor_does_not_change_a_bit(case, monkeypatch):
    from abnet3_amd import _lib
    rng = np.random.default_rng(7)
    if case == 'ties':
        Q, C = tie_case(rng, 300, 1000)
    else:
        C, basis = unit_rows(rng, 1000, 400)
        Q = C[::3].copy()
    qm, cm = random_meta(rng, len(Q)), random_meta(rng, len(C))
    outs, sizes = {}, {}
    for split in ('1', '2', '7', 'auto'):
        monkeypatch.setenv('ABN_KNN_SPLIT', split)
        sizes[split] = _lib.load().abn_knn_ws_bytes(len(Q), len(C), 10)
        outs[split] = gpu_topk(Q, C, 10, qm, cm)
    assert sizes['1'] == 0 and len(set(sizes.values())) == 4            # four different splits really ran
    for split in ('2', '7', 'auto'):
        assert np.array_equal(outs[split][0], outs['1'][0]), split
        assert np.array_equal(outs[split][1].view(np.int32), outs['1'][1].view(np.int32)), split


def planted_corpus(rng, n_files=10, D=40, n_words=5, per_file=4):
    """Noise files with a few "word" templates (smooth 50-frame trajectories) inserted with noise and random linear
    time-warps.  Returns (features dict, times dict, planted {name: [(begin, end, word)]})."""
    templates = [np.cumsum(rng.standard_normal((50, D)), axis=0) for _ in range(n_words)]
    templates = [3.0 * (t - t.mean(0)) / t.std() for t in templates]
    feats, times, planted = {}, {}, {}
    for f in range(n_files):
        n = int(rng.integers(320, 480))
        x = rng.standard_normal((n, D))
        pos, spots = 10, []
        for _ in range(per_file):
            w = int(rng.integers(n_words))
            ln = int(rng.integers(42, 62))
            if pos + ln + 10 > n:
                break
            src = np.linspace(0, 49, ln)
            lo = np.minimum(np.floor(src).astype(int), 48)
            fr = (src - lo)[:, None]
            x[pos:pos + ln] = templates[w][lo] * (1 - fr) + templates[w][lo + 1] * fr + 0.3 * rng.standard_normal((ln, D))
            spots.append((pos, pos + ln, w))
            pos += ln + int(rng.integers(15, 40))
        name = 'file%02d' % f
        feats[name], times[name], planted[name] = x.astype(np.float32), np.arange(n) * 0.01, spots
    return feats, times, planted


def word_of(planted, name, b, e):
    """The planted word that covers at least half of [b, e), or -1."""
    for pb, pe, w in planted[name]:
        if min(e, pe) - max(b, pb) >= 0.5 * (e - b):
            return w
    return -1


def test_miner_end_to_end_on_a_planted_corpus(tmp_path):
    from abnet3_amd.dataloader import PairsDataLoader
    from abnet3_amd.discovery import KnnPairMiner
    rng = np.random.default_rng(3)
    feats, times, planted = planted_corpus(rng)
    k, min_sim = 10, 0.3
    miner = KnnPairMiner(feats, times, lengths=(40, 60), shift=5, frames=10, k=k, min_similarity=min_sim)
    pairs_path, map_path = miner.write(str(tmp_path / 'mined'))
    names = sorted(feats)
    assert miner.names == names
    # the restatement, in float64
    arrays = [feats[n] for n in names]
    segs = knn_np.segments([len(a) for a in arrays], (40, 60), 5)
    assert list(zip(miner.seg_file.tolist(), miner.seg_begin.tolist(), miner.seg_len.tolist())) == segs
    u64, _ = knn_np.unit64(knn_np.gather(arrays, segs, 10))
    meta = np.array([(f, s, s + ln) for f, s, ln in segs], dtype=np.int32)
    S, excl = u64 @ u64.T, knn_np.excluded(meta, meta)
    dlt = knn_np.delta(400)
    knn_np.check_topk(miner.idx, miner.sim, S, k, excl, dlt)
    ref_idx, ref_sim = knn_np.topk(S, k, excl)
    ref = {(a, b): s for a, b, s in knn_np.pairs_from_lists(ref_idx, ref_sim, min_sim, True)}
    mine = {(int(a), int(b)): float(s) for a, b, s in zip(*miner.pairs)}
    # a pair sits near a cut when its similarity is within delta of min_similarity or of either list's k-th place
    tau = ref_sim[:, -1]
    near = lambda a, b: (abs(S[a, b] - min_sim) <= dlt or abs(S[a, b] - tau[a]) <= dlt or abs(S[a, b] - tau[b]) <= dlt)
    for key in set(ref) ^ set(mine):
        assert near(*key), (key, S[key])
    for key in set(ref) & set(mine):
        assert abs(ref[key] - mine[key]) <= dlt
    assert len(mine) > 20
    # the written files
    lines = open(pairs_path).read().splitlines()
    assert len(lines) == len(mine)
    sims = []
    for line in lines:
        fld = line.split(' ')
        assert len(fld) == 7
        f1, f2, b1, e1, b2, e2 = (int(v) for v in fld[:6])
        assert 0 <= b1 < e1 <= len(arrays[f1]) and 0 <= b2 < e2 <= len(arrays[f2])
        assert e1 - b1 in (40, 60) and e2 - b2 in (40, 60)
        assert not (f1 == f2 and b1 < e2 and b2 < e1), line
        sims.append(1.0 - float(fld[6]))
    assert all(a >= b - 1e-10 for a, b in zip(sims, sims[1:]))
    assert open(map_path).read().splitlines() == ['%d %s' % (i, n) for i, n in enumerate(names)]
    dl = PairsDataLoader(pairs_path, None, map_path, split_method='files')
    dl.load_pairs()
    assert dl.files <= set(names)
    # precision of the top pairs against the planted positions (reported).  Chance: the share of ALL admissible
    # segment pairs that cover two instances of one word.
    words = np.array([word_of(planted, names[f], s, s + ln) for f, s, ln in segs])
    same = (words[:, None] == words[None, :]) & (words[:, None] >= 0) & ~excl
    chance = same.sum() / float((~excl).sum())
    top = list(zip(*miner.pairs))[:max(20, len(mine) // 4)]
    precision = np.mean([same[int(a), int(b)] for a, b, _ in top])
    print('planted corpus: %d segments, %d pairs; precision of the top %d: %.3f (chance %.4f)'
          % (len(segs), len(mine), len(top), precision, chance))
    assert precision >= 10 * chance and precision >= 0.5
