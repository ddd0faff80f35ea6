"""The term-discovery prefilter on the MI355X: abn_lsh_signatures against the float64 restatement wherever the float32
error bound decides the sign, `live` exactly; abn_lsh_diag_hits_batched against the restatement (tests/prefilter_np.py)
for exact equality of best, diag and end1 -- the length, span, dilation, threshold and width edges, runs planted on and
across the lane-block edges, dead rows, the exclusion band, ties, empty and refused pairs, the grid-stride loop --, the
Python surface, and TermDiscoverer with a TermPrefilter end to end."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import prefilter_np  # noqa: E402
import terms_np  # noqa: E402

pytestmark = pytest.mark.gpu

CAP = prefilter_np.CAP
N2_EDGES = [1, 2, 63, 64, 65, 127, 128, 129, 511, 512]
N1_EDGES = [1, 5, 64, 65, 200, 700]
SPANS = [1, 2, 32, 63, 64]


def dev(a, dt=None):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()


def dev_sig(sig):
    """uint32 [rows, words] as the int32 device tensor the Python surface holds."""
    return torch.from_numpy(np.ascontiguousarray(sig, dtype=np.uint32).view(np.int32)).cuda()


def offsets(n):
    return np.concatenate(([0], np.cumsum(n)[:-1])).astype(np.int64)


# ---------------------------------------------------------------------------------------------------------------
# signatures

def raw_signatures(table, planes):
    """The entry point alone: the table allocated exactly, the outputs one row longer and prefilled."""
    from abnet3_amd import _lib
    rows, D = table.shape
    bits = planes.shape[0]
    t, p = dev(table, np.float32), dev(planes, np.float32)
    sig = torch.full((rows + 1, bits // 32), 0x5a5a5a5a, dtype=torch.int32, device='cuda')
    live = torch.full((rows + 1,), 7, dtype=torch.uint8, device='cuda')
    _lib.check(_lib.load().abn_lsh_signatures(_lib.ptr(t), rows, D, _lib.ptr(p), bits, _lib.ptr(sig), _lib.ptr(live), _lib.stream()),
               'abn_lsh_signatures')
    torch.cuda.synchronize()
    s, l = sig.cpu().numpy(), live.cpu().numpy()
    assert (s[rows] == 0x5a5a5a5a).all() and l[rows] == 7            # nothing past the last row
    return s[:rows].view(np.uint32), l[:rows]


@pytest.mark.parametrize('bits', [32, 64, 96, 256])
def test_signatures_match_the_restatement_where_the_bound_decides(bits):
    """Every bit equals the float64 sign wherever |dot| exceeds the float32 forward error bound; the entries inside the
    bound -- a property of the inputs, not of the kernel -- are at most 0.1 % of all bits of the case's shapes."""
    rng = np.random.default_rng(bits)
    inside = total = 0
    for D in (1, 3, 40, 41, 100, 280, 500):
        planes = prefilter_np.planes(D, bits, seed=D)
        for rows in (1, 63, 64, 65, 1000):
            table = rng.standard_normal((rows, D)).astype(np.float32)
            if rows >= 63:                                          # dead rows between good ones
                table[3] = 0.0
                table[7, D // 2] = np.nan
                table[20, 0] = np.inf
                table[21, D - 1] = -np.inf
                table[40] = np.nan
                table[rows - 1, D // 3] = np.inf
            ref_sig, ref_live, decided = prefilter_np.signatures(table, planes)
            sig, live = raw_signatures(table, planes)
            assert np.array_equal(live, ref_live), (D, rows)
            alive = ref_live != 0
            assert not sig[~alive].any(), (D, rows)
            if rows >= 63:
                assert (~alive).sum() == 6 and alive[[2, 4, 6, 8, 19, 22, 39, 41, rows - 2]].all()
            got, want = prefilter_np.unpack(sig, bits)[alive], prefilter_np.unpack(ref_sig, bits)[alive]
            sure = decided[alive]
            assert np.array_equal(got[sure], want[sure]), (D, rows, int((got[sure] != want[sure]).sum()))
            inside += int((~sure).sum())
            total += sure.size
    print('entries inside the bound: %d of %d' % (inside, total))
    assert inside <= 1e-3 * total, (inside, total)


def test_lsh_signatures_surface():
    from abnet3_amd.prefilter import lsh_planes, lsh_signatures
    rng = np.random.default_rng(1)
    table = rng.standard_normal((130, 40)).astype(np.float32)
    table[5] = 0.0
    planes = lsh_planes(40, 64, seed=3)
    sig, live = lsh_signatures(dev(table), planes)
    assert sig.is_cuda and sig.dtype == torch.int32 and sig.shape == (130, 2) and live.dtype == torch.uint8 and live.shape == (130,)
    raw_sig, raw_live = raw_signatures(table, planes)
    assert np.array_equal(sig.cpu().numpy().view(np.uint32), raw_sig) and np.array_equal(live.cpu().numpy(), raw_live)
    again, _ = lsh_signatures(dev(table), dev(planes))               # device planes: the same words
    assert torch.equal(again, sig)
    # the same frame scaled keeps its signature, its opposite flips every bit
    pair = np.stack([table[0], 2.5 * table[0], -table[0]]).astype(np.float32)
    s, _ = lsh_signatures(dev(pair), planes)
    s = s.cpu().numpy().view(np.uint32)
    assert np.array_equal(s[0], s[1]) and prefilter_np.popcount(s[0] ^ s[2]).sum() == 64
    empty = lsh_signatures(torch.empty((0, 40), device='cuda'), planes)
    assert empty[0].shape == (0, 2) and empty[1].shape == (0,)
    with pytest.raises(ValueError, match='widths'):
        lsh_signatures(dev(table), lsh_planes(39, 64))
    with pytest.raises(ValueError, match='bits'):
        lsh_signatures(dev(table), rng.standard_normal((48, 40)).astype(np.float32))
    with pytest.raises(ValueError, match='float32'):
        lsh_signatures(dev(table).double(), planes)


# ---------------------------------------------------------------------------------------------------------------
# diagonal hits

def raw_hits(s1, l1, o1, n1, s2, l2, o2, n2, max_hamming, span, dilate, exclude=0):
    """The entry point alone over device tables, the outputs one pair longer and prefilled with 7."""
    from abnet3_amd import _lib
    P = len(n1)
    tab = [dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)]
    out = [torch.full((P + 1,), 7, dtype=torch.int32, device='cuda') for _ in range(3)]
    _lib.check(_lib.load().abn_lsh_diag_hits_batched(
        _lib.ptr(s1), _lib.ptr(l1), s1.shape[0], _lib.ptr(s2), _lib.ptr(l2), s2.shape[0], *[_lib.ptr(x) for x in tab], P,
        s1.shape[1], max_hamming, span, dilate, exclude, *[_lib.ptr(x) for x in out], _lib.stream()), 'abn_lsh_diag_hits_batched')
    torch.cuda.synchronize()
    res = [x.cpu().numpy() for x in out]
    assert all(r[P] == 7 for r in res)                               # nothing past the last pair
    return tuple(r[:P] for r in res)


def assert_same(got, ref, what=''):
    for name, g, r in zip(('best', 'diag', 'end1'), got, ref):
        assert np.array_equal(g, r), (what, name, np.flatnonzero(g != r)[:10], g[g != r][:10], r[g != r][:10])


def pool_table(rng, rows, words, dead=0.03):
    """Signatures drawn from a pool of 8 values -- hits are common -- of which value 1 is value 0 with one bit flipped,
    value 2 with bits / 4 flipped and value 3 with bits / 4 + 1; some rows dead."""
    bits = 32 * words
    pool = rng.integers(0, 1 << 32, (8, words), dtype=np.uint64).astype(np.uint32)

    def flipped(k):
        out = pool[0].copy()
        for b in rng.choice(bits, k, replace=False):
            out[b // 32] ^= np.uint32(1) << np.uint32(b % 32)
        return out
    pool[1], pool[2], pool[3] = flipped(1), flipped(bits // 4), flipped(bits // 4 + 1)
    return pool[rng.integers(0, 8, rows)], (rng.random(rows) >= dead).astype(np.uint8)


def check(sig1, live1, o1, n1, sig2, live2, o2, n2, max_hamming, span, dilate, exclude=0, what='', same=False):
    ref = prefilter_np.diag_hits(sig1, live1, o1, n1, sig2, live2, o2, n2, max_hamming, span, dilate, exclude)
    s1, l1 = dev_sig(sig1), dev(live1, np.uint8)
    s2, l2 = (s1, l1) if same else (dev_sig(sig2), dev(live2, np.uint8))
    got = raw_hits(s1, l1, o1, n1, s2, l2, o2, n2, max_hamming, span, dilate, exclude)
    assert_same(got, ref, what)
    return got


@pytest.mark.parametrize('dilate', [0, 1, 8])
@pytest.mark.parametrize('words', [1, 2, 8])
def test_length_span_and_threshold_edges(words, dilate):
    """Every side-2 edge against every side-1 edge in one pair table, once per span; the thresholds 0, 1, bits / 4 and
    bits take turns (each of them meets the dilation and the width of the case)."""
    rng = np.random.default_rng(100 * words + dilate)
    bits = 32 * words
    n1 = np.repeat(N1_EDGES, len(N2_EDGES)).astype(np.int32)
    n2 = np.tile(N2_EDGES, len(N1_EDGES)).astype(np.int32)
    o1, o2 = offsets(n1), offsets(n2)
    sig1, live1 = pool_table(rng, int(n1.sum()), words)
    sig2, live2 = pool_table(rng, int(n2.sum()), words)
    sig2[:] = sig1[rng.integers(0, len(sig1), len(sig2))]            # the same pool on both sides
    thresholds = [0, 1, bits // 4, bits]
    bests = []
    for k, span in enumerate(SPANS):
        mh = thresholds[(k + dilate + words) % 4]
        got = check(sig1, live1, o1, n1, sig2, live2, o2, n2, mh, span, dilate, what=(span, mh))
        assert (got[0] >= 0).all() and (got[0] <= np.minimum(span, np.minimum(n1, n2))).all()
        hit = got[0] > 0
        assert ((got[2][hit] >= 0) & (got[2][hit] < n1[hit])).all()
        j = got[2][hit] - got[1][hit]
        assert ((j >= 0) & (j < n2[hit])).all() and (got[2][~hit] == -1).all() and (got[1][~hit] == 0).all()
        bests.append(got[0])
    assert all((b > 0).any() for b in bests) and len({int(b.max()) for b in bests}) >= 3
    # the two ends of the threshold at one span: no fewer hits with the wider one, and at `bits` every live pair hits
    narrow, wide = (check(sig1, live1, o1, n1, sig2, live2, o2, n2, mh, 32, dilate, what=('mh', mh))[0] for mh in (0, bits))
    full = np.minimum(32, np.minimum(n1, n2))
    assert (narrow <= wide).all() and (narrow < wide).any() and (wide <= full).all() and (wide == full).sum() >= 10


def unique_table(rng, rows, words=2):
    """Signatures that do not repeat and are far from each other (random 64 bits: ~32 bits apart)."""
    return rng.integers(0, 1 << 32, (rows, words), dtype=np.uint64).astype(np.uint32), np.ones(rows, np.uint8)


@pytest.mark.parametrize('dilate', [0, 1, 8])
def test_runs_planted_on_and_across_the_lane_block_edges(dilate):
    """A run of 40 frames planted on diagonals -1, 0, 62 .. 65 and on both sides of the kernel's own block edges
    (blocks of 64 - 2 dilate diagonals from -(n2 - 1)); straight, and drifting by +-dilate columns half way, across the
    edge; with a dead row inside.  Nothing else hits."""
    rng = np.random.default_rng(40 + dilate)
    N1, N2, L = 260, 150, 40
    U = 64 - 2 * dilate
    edges = sorted({-1, 0, 62, 63, 64, 65} | {k for b in range(1, 8) for k in (-(N2 - 1) + b * U - 1, -(N2 - 1) + b * U) if -90 <= k <= 200})
    assert len(edges) >= 14
    cases = [(k, drift, kill) for k in edges for drift in sorted({0, dilate, -dilate}) for kill in (False, True)]
    P = len(cases)
    sig1, live1 = unique_table(rng, P * N1)
    sig2, live2 = unique_table(rng, P * N2)
    want = []
    for p, (k, drift, kill) in enumerate(cases):
        j0 = 10 - min(k, 0)
        i0 = j0 + k                                                 # the run starts at (i0, j0) on diagonal k
        assert i0 >= 0 and i0 + L <= N1 and j0 + L + 8 <= N2 and j0 - 8 >= 0
        for s in range(L):
            sig2[p * N2 + j0 + s + (drift if s >= L // 2 else 0)] = sig1[p * N1 + i0 + s]
        if kill:
            live1[p * N1 + i0 + 5] = 0
        # straight, or drifting `dilate` columns to the right half way (onto diagonal k - dilate): the dilation spreads the
        # run over the neighbouring diagonals, the smallest one that sees all 40 rows is k - dilate, and 32 of them fill
        # the window first at row i0 + 31 -- around the dead row, at i0 + 37.  A drift to the LEFT writes over the first
        # half's last columns: those cases are held against the restatement only
        want.append((32, k - dilate, i0 + (37 if kill else 31)) if drift >= 0 else None)
    o1, o2 = np.arange(P, dtype=np.int64) * N1, np.arange(P, dtype=np.int64) * N2
    n1, n2 = np.full(P, N1, np.int32), np.full(P, N2, np.int32)
    got = check(sig1, live1, o1, n1, sig2, live2, o2, n2, 0, 32, dilate, what='planted')
    assert all(w is None or tuple(int(g[p]) for g in got) == w for p, w in enumerate(want)) and sum(w is not None for w in want) >= 2 * len(edges)
    if dilate:                                                       # without the dilation a drifting run is two halves of 20
        flat = check(sig1, live1, o1, n1, sig2, live2, o2, n2, 0, 32, 0, what='planted, no dilation')
        drifting = np.array([c[1] != 0 for c in cases])
        assert (flat[0][drifting] <= 20).all() and (flat[0][~drifting] == 32).all()
    long_ = check(sig1, live1, o1, n1, sig2, live2, o2, n2, 0, 64, dilate, what=('planted', 64))      # the whole run in one window
    assert all(long_[0][p] == (39 if c[2] else 40) for p, c in enumerate(cases) if c[1] >= 0)


def test_ties_between_and_inside_diagonals():
    rng = np.random.default_rng(7)
    N1, N2 = 200, 140
    sig1, live1 = unique_table(rng, 3 * N1)
    sig2, live2 = unique_table(rng, 3 * N2)
    # pair 0: two runs of 20 on diagonals 70 and -30 (two lane blocks, two wavefronts): the smaller diagonal
    sig2[5:25] = sig1[75:95]
    sig2[100:120] = sig1[70:90]
    # pair 1: two runs of 20 on ONE diagonal (10), 45 rows apart: the smaller row
    sig2[N2 + 20:N2 + 40] = sig1[N1 + 30:N1 + 50]
    sig2[N2 + 65:N2 + 85] = sig1[N1 + 75:N1 + 95]
    # pair 2: equal runs on neighbouring diagonals 63 and 64
    sig2[2 * N2 + 10:2 * N2 + 22] = sig1[2 * N1 + 74:2 * N1 + 86]
    sig2[2 * N2 + 50:2 * N2 + 62] = sig1[2 * N1 + 113:2 * N1 + 125]
    o1, o2 = np.arange(3, dtype=np.int64) * N1, np.arange(3, dtype=np.int64) * N2
    n1, n2 = np.full(3, N1, np.int32), np.full(3, N2, np.int32)
    got = check(sig1, live1, o1, n1, sig2, live2, o2, n2, 0, 32, 0, what='ties')
    assert [tuple(int(g[p]) for g in got) for p in range(3)] == [(20, -30, 89), (20, 10, 49), (12, 63, 124)]
    got = check(sig1, live1, o1, n1, sig2, live2, o2, n2, 0, 64, 0, what='ties, span 64')
    assert [tuple(int(g[p]) for g in got) for p in range(3)] == [(20, -30, 89), (39, 10, 93), (12, 63, 124)]


@pytest.mark.parametrize('exclude', [1, 50])
def test_exclusion_on_one_table(exclude):
    """Utterances against themselves and against shifted windows of themselves in ONE table: the band follows the table
    rows.  Each utterance holds a repeat of 30 of its frames 80 rows further on."""
    rng = np.random.default_rng(60 + exclude)
    n = np.array([200, 65, 600, 130], np.int32)
    base = offsets(n)
    sig, live = unique_table(rng, int(n.sum()))
    for b, ln in zip(base, n):
        if ln >= 130:
            sig[b + 90:b + 120] = sig[b + 10:b + 40]
    rows = [(u, w0, wn) for u, ln in enumerate(n) for w0, wn in terms_np.windows(int(ln), 128)] + \
           [(u, w0, min(int(n[u]) - w0, 77)) for u in range(4) for w0 in (1, 49, 50, 51)]
    o1, n1 = np.array([base[u] for u, _, _ in rows]), np.array([n[u] for u, _, _ in rows], np.int32)
    o2, n2 = np.array([base[u] + w0 for u, w0, _ in rows]), np.array([wn for _, _, wn in rows], np.int32)
    for span, dilate in ((32, 0), (64, 1), (5, 8)):
        got = check(sig, live, o1, n1, sig, live, o2, n2, 0, span, dilate, exclude=exclude, what=(span, dilate), same=True)
        hit = got[0] > 0
        gap = (o1 + got[2]) - (o2 + got[2] - got[1])
        assert (np.abs(np.abs(gap[hit]) - 80) <= dilate).all() and hit.sum() >= 6         # the repeat, never the main diagonal
    free = check(sig, live, o1, n1, sig, live, o2, n2, 0, 32, 0, what='no exclusion', same=True)
    assert (free[0] == np.minimum(32, n2)).all() and ((o1 + free[2]) == (o2 + free[2] - free[1])).all()
    from abnet3_amd import _lib
    s, l = dev_sig(sig), dev(live, np.uint8)
    with pytest.raises(_lib.HipLibraryError, match='one table'):
        raw_hits(s, l, o1, n1, s.clone(), l, o2, n2, 0, 32, 0, exclude=exclude)


def test_refusals_and_empty_sides_between_good_pairs():
    """n2 = 513, negative lengths, offsets past the end and far outside: -1, the neighbours right, nothing read -- the
    tables are allocated exactly."""
    rng = np.random.default_rng(9)
    rows1, rows2 = 700, CAP + 1
    sig1, live1 = pool_table(rng, rows1, 2)
    sig2, live2 = pool_table(rng, rows2, 2)
    sig2[:] = sig1[rng.integers(0, rows1, rows2)]
    good = (0, 700, 0, CAP)
    far = 2 ** 40
    int32_max = 2 ** 31 - 1
    bad = [(0, 10, 0, CAP + 1), (0, -1, 0, 3), (0, 3, 0, -5), (rows1 - 3, 4, 0, 3), (0, 3, rows2 - 1, 3), (rows1 + 1, 0, 0, 1),
           (far, 3, 0, 3), (0, 3, -far, 3), (-1, 3, 0, 3), (2 ** 62, int32_max, 0, 3), (0, 3, 2 ** 63 - 1, 1), (0, int32_max, 0, 3)]
    table = []
    for b in bad:
        table += [good, b]
    empty = [(5, 0, 5, 10), (5, 10, 5, 0), (rows1, 0, rows2, 0), (0, 0, 0, 0)]
    table += [good] + empty + [(rows1 - 3, 3, rows2 - 2, 2)]         # legal: empty sides (at the very end too), flush with the end
    o1, n1, o2, n2 = (np.array(c) for c in zip(*table))
    got = check(sig1, live1, o1, n1.astype(np.int32), sig2, live2, o2, n2.astype(np.int32), 16, 32, 1, what='refusals')
    k = 2 * len(bad)
    assert (got[0][1:k:2] == -1).all() and (got[1][1:k:2] == 0).all() and (got[2][1:k:2] == -1).all()
    assert (got[0][0:k + 1:2] == got[0][0]).all() and got[0][0] > 0 and (got[2][0:k + 1:2] == got[2][0]).all()
    assert got[0][k + 1:k + 5].tolist() == [0] * 4 and got[2][k + 1:k + 5].tolist() == [-1] * 4 and got[0][-1] >= 0


def test_more_pairs_than_one_pass_of_the_grid_and_none():
    from abnet3_amd import _lib
    from abnet3_amd.prefilter import GRID_BLOCKS
    rng = np.random.default_rng(10)
    K = 300
    n1, n2 = rng.integers(0, 12, K).astype(np.int32), rng.integers(0, 9, K).astype(np.int32)
    sig1, live1 = pool_table(rng, int(n1.sum()), 1, dead=0.1)
    sig2, live2 = pool_table(rng, int(n2.sum()), 1, dead=0.1)
    sig2[:] = sig1[rng.integers(0, len(sig1), len(sig2))]
    o1, o2 = offsets(n1), offsets(n2)
    ref = prefilter_np.diag_hits(sig1, live1, o1, n1, sig2, live2, o2, n2, 1, 4, 1)
    assert (ref[0] > 1).sum() > 50 and (ref[0] == 0).sum() > 5
    pick = rng.integers(0, K, 2 * GRID_BLOCKS + 1001)
    s1, l1, s2, l2 = dev_sig(sig1), dev(live1, np.uint8), dev_sig(sig2), dev(live2, np.uint8)
    got = raw_hits(s1, l1, o1[pick], n1[pick], s2, l2, o2[pick], n2[pick], 1, 4, 1)
    assert_same(got, tuple(r[pick] for r in ref), 'grid stride')
    none = np.zeros(0, np.int64)
    assert all(len(r) == 0 for r in raw_hits(s1, l1, none, none, s2, l2, none, none, 1, 4, 1))
    assert _lib.load().abn_lsh_diag_hits_batched(_lib.ptr(s1), _lib.ptr(l1), len(sig1), _lib.ptr(s2), _lib.ptr(l2), len(sig2), None,
                                                 None, None, None, 0, 1, 1, 4, 1, 0, None, None, None, None) == 0


def test_diag_hits_batch_surface():
    from abnet3_amd.prefilter import diag_hits_batch
    rng = np.random.default_rng(11)
    sig, live = pool_table(rng, 400, 2)
    s, l = dev_sig(sig), dev(live, np.uint8)
    o1, n1, o2, n2 = [0, 100, 0, 390], [300, 40, 10, 20], [0, 1, 5, 0], [200, 7, 0, CAP + 1]
    ref = prefilter_np.diag_hits(sig, live, o1, n1, sig, live, o2, n2, 16, 32, 1)
    out = diag_hits_batch(s, l, o1, n1, s, l, o2, n2, 16, span=32, dilate=1)
    assert len(out) == 3 and all(t.is_cuda and t.dtype == torch.int32 and t.shape == (4,) for t in out)
    assert_same(tuple(t.cpu().numpy() for t in out), ref)
    assert out[0].tolist()[2:] == [0, -1]                             # an empty side; a refused pair comes back as -1
    out = diag_hits_batch(s, l, dev(o1, np.int64), dev(n1, np.int32), s, l, dev(o2, np.int64), dev(n2, np.int32), 16, 32, 1)
    assert_same(tuple(t.cpu().numpy() for t in out), ref, 'device columns')
    ref = prefilter_np.diag_hits(sig, live, o1, n1, sig, live, o2, n2, 16, 32, 0, exclude=30)
    assert_same(tuple(t.cpu().numpy() for t in diag_hits_batch(s, l, o1, n1, s, l, o2, n2, 16, exclude=30)), ref, 'exclude')
    assert all(t.numel() == 0 for t in diag_hits_batch(s, l, [], [], s, l, [], [], 16))
    with pytest.raises(ValueError, match='same table'):
        diag_hits_batch(s, l, o1, n1, s.clone(), l, o2, n2, 16, exclude=3)
    with pytest.raises(ValueError, match='same table'):
        diag_hits_batch(s, l, o1, n1, s, l.clone(), o2, n2, 16, exclude=3)
    with pytest.raises(ValueError, match='width'):
        diag_hits_batch(s, l, o1, n1, s[:, :1].contiguous(), l, o2, n2, 16)
    with pytest.raises(ValueError, match='lsh_signatures'):
        diag_hits_batch(s.float(), l, o1, n1, s, l, o2, n2, 16)
    with pytest.raises(ValueError, match='lsh_signatures'):
        diag_hits_batch(s, l[:-1], o1, n1, s, l, o2, n2, 16)
    for kw, name in ((dict(max_hamming=65), 'max_hamming'), (dict(max_hamming=-1), 'max_hamming'), (dict(span=0), 'span'),
                     (dict(span=65), 'span'), (dict(dilate=9), 'dilate'), (dict(dilate=-1), 'dilate'), (dict(exclude=-1), 'exclude')):
        args = dict(max_hamming=16)
        args.update(kw)
        with pytest.raises(ValueError, match=name):
            diag_hits_batch(s, l, o1, n1, s, l, o2, n2, **args)
    with pytest.raises(ValueError, match='differ in length'):
        diag_hits_batch(s, l, o1, n1[:-1], s, l, o2, n2, 16)


# ---------------------------------------------------------------------------------------------------------------
# end to end

def end_to_end_prefilter():
    from abnet3_amd.prefilter import TermPrefilter
    return TermPrefilter(bits=64, seed=1, max_hamming=16, span=32, dilate=0, min_hits=24)


def written(td, out_dir):
    return [open(p, 'rb').read() for p in td.write(str(out_dir))]


def producing(td, kp):
    """The kernel pairs that give a kept match on their own."""
    from abnet3_amd.terms import keep_matches
    res = td.align(kp)
    return np.array([bool(keep_matches([q], [r[p:p + 1] for r in res], td.theta, td.min_frames, td.max_distance))
                     for p, q in enumerate(kp)])


def restated_mask(td, pre, kp):
    sig, live = (x.cpu().numpy() for x in pre.signatures(td))
    base = [td.corpus.offset[k] for k in td.names]
    lengths = [td.corpus.length[k] for k in td.names]
    best = prefilter_np.best_runs(sig.view(np.uint32), live, base, lengths, kp, td.exclude, pre.max_hamming, pre.span, pre.dilate)
    return best, prefilter_np.keep(best, pre.min_hits)


def test_discoverer_with_the_prefilter_end_to_end(tmp_path):
    from abnet3_amd.terms import TermDiscoverer, kernel_pairs
    feats, times, words = terms_np.planted_corpus()
    names = sorted(feats)
    plain = TermDiscoverer(feats, times, theta=0.05)
    m0, c0 = plain.discover()
    assert plain.n_kernel_pairs == plain.n_aligned_pairs == 18 and plain.prefilter_best is None
    files0 = written(plain, tmp_path / 'plain')
    pre = end_to_end_prefilter()
    td = TermDiscoverer(feats, times, theta=0.05)
    m1, c1 = td.discover(prefilter=pre)
    assert m1 == m0 and c1 == c0 and len(c0) == len(words)
    kp = kernel_pairs([len(feats[k]) for k in names], terms_np.all_pairs(len(names)), td.window)
    best, mask = restated_mask(td, pre, kp)
    assert td.prefilter_best.dtype == np.int32 and np.array_equal(td.prefilter_best, best)
    assert np.array_equal(td.prefilter_best >= pre.min_hits, mask)
    assert (td.n_kernel_pairs, td.n_aligned_pairs) == (18, int(mask.sum())) and td.n_aligned_pairs < td.n_kernel_pairs / 2
    assert int(mask.sum()) == 7 and (best[mask] == 32).all() and best[~mask].max() <= 17
    assert mask[producing(plain, kp)].all()
    files1 = written(td, tmp_path / 'pre')
    assert files1[0] == files0[0] and files1 == files0                # terms.classes byte for byte (and the pair files)
    # the constructor's prefilter, small launches, and the signatures built once per discoverer
    td5 = TermDiscoverer(feats, times, theta=0.05, chunk_pairs=5, prefilter=pre)
    assert td5.discover() == (m0, c0) and np.array_equal(td5.prefilter_best, best)
    first = pre.signatures(td5)[0]
    td5.discover()
    assert pre.signatures(td5)[0] is first
    assert td5.discover(pairs=[('utt1', 'utt2'), ('utt4', 'utt3')])[0] == plain.discover(pairs=[('utt1', 'utt2'), ('utt4', 'utt3')])[0]


def test_discoverer_with_the_prefilter_over_posteriorgrams():
    from abnet3_amd.terms import TermDiscoverer, kernel_pairs
    feats, times, words = terms_np.planted_corpus()
    names = sorted(feats)
    post = {}
    for k, v in feats.items():                                      # a row softmax: copies stay copies
        e = np.exp(v - v.max(axis=1, keepdims=True))
        post[k] = (e / e.sum(axis=1, keepdims=True)).astype(np.float32)
    post['utt3'][300, 3] = -0.5                                     # a BAD row: dead in the signatures
    plain = TermDiscoverer(post, times, distance='kl', theta=0.05)
    m0, c0 = plain.discover()
    pre = end_to_end_prefilter()
    td = TermDiscoverer(post, times, distance='kl', theta=0.05, prefilter=pre)
    assert td.discover() == (m0, c0) and len(c0) == len(words)
    kp = kernel_pairs([len(post[k]) for k in names], terms_np.all_pairs(len(names)), td.window)
    mask = td.prefilter_best >= pre.min_hits
    assert mask[producing(plain, kp)].all() and td.n_aligned_pairs == int(mask.sum()) <= td.n_kernel_pairs == 18
    best, restated = restated_mask(td, pre, kp)
    assert np.array_equal(td.prefilter_best, best) and np.array_equal(mask, restated)
    sig, live = pre.signatures(td)
    bad_row = td.corpus.offset['utt3'] + 300
    assert td.tables.bad[bad_row].item() == 1 and live[bad_row].item() == 0 and not sig[bad_row].any().item()
    assert int(live.sum().item()) == len(live) - 1
    # the signatures are those of sqrt(P) under the planes of (seed, bits, D)
    ref_sig, ref_live, decided = prefilter_np.signatures(np.sqrt(td.tables.P.cpu().numpy()), prefilter_np.planes(40, 64, seed=1))
    got = prefilter_np.unpack(sig.cpu().numpy().view(np.uint32), 64)
    alive = live.cpu().numpy() != 0
    sure = decided & alive[:, None]
    assert np.array_equal(got[sure], prefilter_np.unpack(ref_sig, 64)[sure]) and sure.mean() > 0.99
