"""The max-product path of the sticky HMM on the host: the numpy restatement (tests/hmm_vit_np.py) against enumeration of
all paths, its special cases and tie rules, its relation to the sum-product likelihood, and everything the library and
the Python layer refuse before a launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_np  # noqa: E402
import hmm_vit_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_hmm_viterbi', 'abn_hmm_viterbi_ws_bytes')
STAYS = (0.0, 0.3, 0.9, 0.999)


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def small_cases():
    """K = 1 .. 3, up to 6 frames; a BAD frame in the middle, at the start and at the end."""
    rng = np.random.default_rng(11)
    out = []
    for K in (1, 2, 3):
        for L in (1, 2, 4, 6):
            for where in (None, 'middle', 'start', 'end'):
                logn = rng.normal(size=(L, K)) * 2.0
                bad = np.zeros(L, dtype=bool)
                if where == 'middle':
                    bad[L // 2] = True
                elif where == 'start':
                    bad[0] = True
                elif where == 'end':
                    bad[-1] = True
                out.append((logn, bad, rng.dirichlet(np.ones(K)).astype(np.float32)))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('stay', STAYS)
def test_float64_restatement_attains_the_brute_force_maximum(stay):
    for logn, bad, w in small_cases():
        good = ~bad
        n = int(good.sum())
        best, arg = hmm_vit_np.brute_force(logn, bad, w, stay)
        # unrounded tables: the recurrence IS the enumeration's maximum, to float64 rounding
        t64 = hmm_vit_np.tables(w, stay, np.float64)
        ids, lp, nsw, ng = hmm_vit_np.viterbi_one(logn, good, *t64, dtype=np.float64)
        tol = 1e-12 * (abs(best) + 1.0)
        assert abs(lp - best) <= tol and ng == n
        assert abs(hmm_vit_np.J(logn, ids, good, *t64) - best) <= tol                 # its path attains it
        assert abs(hmm_vit_np.optimum_f64(logn, good, *t64) - best) <= tol
        assert (ids[bad] == -1).all() and (ids[good] >= 0).all()
        if len(arg) == 1 and n:
            assert tuple(ids[good]) == arg[0]
        assert nsw == hmm_vit_np.switches(ids)
        # the float32 tables: one rounding of one table entry per good frame
        t32 = hmm_vit_np.tables(w, stay)
        assert all(t.dtype == np.float32 for t in t32)
        lp32 = hmm_vit_np.viterbi_one(logn, good, *t32, dtype=np.float64)[1]
        assert abs(lp32 - best) <= n * hmm_vit_np.U * hmm_vit_np.table_max(*t32) + tol


def test_zero_stay_is_the_frame_wise_argmax():
    rng = np.random.default_rng(2)
    s = (rng.normal(size=(50, 7)) * 3.0).astype(np.float32)
    good = rng.random(50) > 0.1
    w = rng.dirichlet(np.ones(7))
    lw, ls, lr = hmm_vit_np.tables(w, 0.0)
    assert np.array_equal(lw, ls) and np.array_equal(lw, lr)
    ids, lp, nsw, ng = hmm_vit_np.viterbi_one(s, good, lw, ls, lr)
    u = (s + lw).astype(np.float32)
    assert np.array_equal(ids[good], np.argmax(u, axis=1)[good]) and (ids[~good] == -1).all()
    assert lp == float(u.max(axis=1)[good].astype(np.float64).sum()) and ng == int(good.sum())


def test_a_component_of_weight_zero_is_never_chosen():
    rng = np.random.default_rng(3)
    s = rng.normal(size=(40, 4)).astype(np.float32)
    s[:, 2] += 50.0                                                     # by far the largest emission
    w = np.array([0.5, 0.3, 0.0, 0.2])
    for stay in STAYS:
        lw, ls, lr = hmm_vit_np.tables(w, stay)
        assert lw[2] == -np.inf and lr[2] == -np.inf
        ids, lp, _, _ = hmm_vit_np.viterbi_one(s, np.ones(40, dtype=bool), lw, ls, lr)
        assert (ids != 2).all() and (ids >= 0).all() and np.isfinite(lp)


def test_tie_rules_lowest_index_and_switch_on_an_exact_tie():
    z = np.zeros(3, dtype=np.float32)
    # all equal: the lowest index in every frame
    ids, lp, nsw, _ = hmm_vit_np.viterbi_one(np.zeros((4, 3), dtype=np.float32), np.ones(4, dtype=bool), z, z, z)
    assert ids.tolist() == [0, 0, 0, 0] and nsw == 0 and lp == 0.0
    # W[k] + ls[k] == lr[k] exactly: not a stay.  Frame 0 leaves W = (0, -1); with ls = 0, lr = -1, component 1's
    # a = -1 equals lr: it switches, and its recorded predecessor is frame 0's j* = 0
    s = np.array([[0.0, -1.0], [0.0, 5.0]], dtype=np.float32)
    ls, lr = np.zeros(2, dtype=np.float32), np.full(2, -1.0, dtype=np.float32)
    ids, lp, nsw, _ = hmm_vit_np.viterbi_one(s, np.ones(2, dtype=bool), np.zeros(2, dtype=np.float32), ls, lr)
    assert ids.tolist() == [0, 1] and nsw == 1 and lp == 4.0
    # one ulp above the tie it stays
    s2 = s.copy()
    s2[0, 1] = np.nextafter(np.float32(-1.0), np.float32(0.0))
    ids, _, nsw, _ = hmm_vit_np.viterbi_one(s2, np.ones(2, dtype=bool), np.zeros(2, dtype=np.float32), ls, lr)
    assert ids.tolist() == [1, 1] and nsw == 0


@pytest.mark.parametrize('stay', STAYS)
def test_log_prob_is_bracketed_by_the_sum_product_likelihood(stay):
    rng = np.random.default_rng(4)
    for K, L in ((2, 30), (5, 60), (9, 25)):
        logn = rng.normal(size=(L, K)) * 2.0
        bad = rng.random(L) < 0.15
        w = rng.dirichlet(np.ones(K)).astype(np.float32)
        t32 = hmm_vit_np.tables(w, stay)
        ids, lp, nsw, ng = hmm_vit_np.viterbi_one(logn, ~bad, *t32, dtype=np.float64)
        ll = hmm_np.forward_backward(logn, bad, w, stay)['loglik']
        slack = ng * hmm_vit_np.U * hmm_vit_np.table_max(*t32) + 1e-9        # the float32 tables against the model's own
        assert lp <= ll + slack and lp >= ll - ng * np.log(K) - slack, (K, L, lp, ll)
        assert nsw == hmm_vit_np.switches(ids)


def test_utterances_in_another_order_give_the_same_rows():
    rng = np.random.default_rng(5)
    lens = np.array([5, 0, 17, 1, 9])
    off = np.cumsum(lens + 2) - lens
    T = int(off[-1] + lens[-1] + 2)
    s = rng.normal(size=(T, 6)).astype(np.float32) * 2.0
    good = rng.random(T) > 0.1
    t32 = hmm_vit_np.tables(rng.dirichlet(np.ones(6)), 0.8)
    ids, lp, nsw, ng = hmm_vit_np.viterbi(s, good, off, lens, *t32)
    perm = np.array([3, 0, 4, 2, 1])
    ids2, lp2, nsw2, ng2 = hmm_vit_np.viterbi(s, good, off[perm], lens[perm], *t32)
    assert np.array_equal(ids, ids2) and np.array_equal(lp[perm], lp2) and np.array_equal(nsw[perm], nsw2)
    assert np.array_equal(ng[perm], ng2) and ng.tolist() == [int(good[o:o + n].sum()) for o, n in zip(off, lens)]
    inside = np.zeros(T, dtype=bool)
    for o, n in zip(off, lens):
        inside[o:o + n] = True
    assert (ids[~inside] == -7).all() and (ids[inside & ~good] == -1).all()
    for u, (o, n) in enumerate(zip(off, lens)):
        assert nsw[u] == hmm_vit_np.switches(ids[o:o + n])


# ---- the Python layer ----------------------------------------------------------------------------------------------------
def test_viterbi_tables_are_the_restatement(lib):
    from abnet3_amd import hmm
    rng = np.random.default_rng(6)
    w = rng.dirichlet(np.ones(9))
    w[4] = 0.0
    w /= w.sum()
    for stay in STAYS + (0.9999,):
        got, ref = hmm.viterbi_tables(w, stay), hmm_vit_np.tables(w, stay)
        for a, b in zip(got, ref):
            assert a.dtype == np.float32 and a.shape == (9,) and np.array_equal(a, b)
        lw, ls, lr = got
        assert lw[4] == -np.inf and lr[4] == -np.inf and (lr <= ls).all() and (lw <= 0).all()
        live = w > 0
        w32, r = w.astype(np.float32).astype(np.float64), np.float64(np.float32(stay))
        omr = np.float64(np.float32(1.0) - np.float32(stay))
        assert np.allclose(np.exp(ls[live].astype(np.float64)), r + omr * w32[live], rtol=1e-6, atol=0)
        assert np.allclose(np.exp(lr[live].astype(np.float64)), omr * w32[live], rtol=1e-6, atol=0)
    assert all(np.array_equal(a, got0) for a, got0 in zip(hmm.viterbi_tables(w, 0.0)[1:], hmm.viterbi_tables(w, 0.0)[:2]))
    for bad in (-0.1, 1.0, float('nan'), 'x'):
        with pytest.raises(ValueError, match='stay'):
            hmm.viterbi_tables(w, bad)
    with pytest.raises(ValueError, match='weights'):
        hmm.viterbi_tables(np.zeros(3), 0.5)
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.viterbi_tables(np.array([1.0, 2.0 ** -100]), 0.5)


def test_viterbi_refuses_on_the_host(lib):
    from abnet3_amd import hmm
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    lw, ls, lr = (torch.from_numpy(a) for a in hmm.viterbi_tables(np.full(K, 1.0 / K), 0.5))
    ninf = float('-inf')
    args = lambda **kw: dict(dict(table=z(6, D), off=[0, 3], lens=[3, 3], shift=z(D), A=z(K, D), B=z(K, D), c0=z(K),
                                  lw=lw, ls=ls, lr=lr), **kw)
    cases = (
        (dict(table=z(6, D).double()), 'float32'), (dict(table=z(6)), 'float32 table'), (dict(A=z(K, D + 1)), 'A \\[K, D\\]'),
        (dict(shift=z(D).double()), 'float32'), (dict(lw=lw.double()), 'lw, ls, lr'), (dict(ls=z(K + 1)), 'lw, ls, lr'),
        (dict(lr=lr.numpy()), 'lw, ls, lr'),
        (dict(lr=ls + 0.5), 'lr <= ls'),
        (dict(lw=torch.tensor([ninf, -1.0, -1.0])), 'same components'), (dict(lr=torch.tensor([ninf, -2.0, -2.0])), 'same components'),
        (dict(lw=torch.full((K,), ninf), lr=torch.full((K,), ninf)), 'everywhere'),
        (dict(ls=torch.tensor([ninf, -0.5, -0.5]), lr=torch.tensor([ninf, -2.0, -2.0])), 'same components'),
        (dict(ls=torch.tensor([ninf, -0.5, -0.5])), 'finite'),
        (dict(ls=torch.tensor([float('nan'), -0.5, -0.5])), 'NaN'), (dict(lw=torch.tensor([float('inf'), -0.5, -0.5])), 'NaN'),
        (dict(lens=[3]), 'offsets'), (dict(lens=[3, 4]), 'outside'), (dict(off=[-1, 3]), 'outside'), (dict(off=[0, 2]), 'overlap'),
        (dict(ids=torch.zeros(6, dtype=torch.int64)), 'ids'), (dict(ids=torch.zeros(5, dtype=torch.int32)), 'ids'),
        (dict(table=z(hmm.max_len() + 1, D), off=[0], lens=[hmm.max_len() + 1]), 'abn_hmm_max_len'),
    )
    for kw, match in cases:
        with pytest.raises(ValueError, match=match):
            hmm.viterbi(**args(**kw))
    Kbig = hmm.max_k() + 1
    big = torch.zeros(Kbig)
    with pytest.raises(ValueError, match='abn_hmm_max_k'):
        hmm.viterbi(z(6, D), [0], [6], z(D), z(Kbig, D), z(Kbig, D), big, big, big, big)
    # a component of weight 0 at stay = 0 (ls = -inf there too) is a valid set of tables
    dead = torch.tensor([ninf, -0.7, -0.7])
    assert hmm._check_log_tables('t', dead, dead, dead, K) is None
    assert hmm._check_log_tables('t', *(torch.from_numpy(a) for a in hmm.viterbi_tables([0.0, 0.5, 0.5], 0.0)), K) is None


def test_class_refuses_on_the_host(lib):
    from abnet3_amd import hmm
    from test_hmm_host import fitted_mixture
    h = hmm.StickyHmmPosteriorgram(fitted_mixture(), 0.75)
    assert h.last_log_prob_ is None and h.last_n_switch_ is None and h.last_n_good_ is None
    for call in (h.decode, h.quantize):
        with pytest.raises(ValueError, match='D = 4'):
            call(torch.zeros(5, 4))
        with pytest.raises(ValueError, match='float32'):
            call(torch.zeros(5, 2, dtype=torch.float64))


# ---- the library -------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_names(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20


def test_sizing_query_and_refusals(lib):
    ws = lib.abn_hmm_viterbi_ws_bytes
    up = lambda v: (v + 255) // 256 * 256

    def layout(n_utt, max_len, K):
        """Per workgroup (one per utterance, 256 at most): 128 x (K rounded up to 128) fp32 scores, and per frame one stay
        bit per component (64-bit words, 4 per 256 components rounded up to a power of two) and an int32."""
        nq = 1
        while nq * 256 < K:
            nq *= 2
        return min(n_utt, 256) * up(128 * ((K + 127) // 128 * 128) * 4 + max_len * (8 * 4 * nq + 4))
    for n_utt, max_len, K, D in ((1, 1, 1, 1), (3, 300, 129, 40), (5000, 1000, 1024, 100), (256, 0, 300, 8), (257, 130, 4096, 127)):
        assert ws(n_utt, max_len, K, D) == layout(n_utt, max_len, K), (n_utt, max_len, K, D)
    # no T x K array: 1.14 M frames in utterances of up to 1000 frames, K = 1024
    assert ws(2000, 1000, 1024, 40) < 1140000 * 1024 * 4 // 8
    for args in ((0, 10, 4, 4), (1 << 31, 10, 4, 4), (1, -1, 4, 4), (1, lib.abn_hmm_max_len() + 1, 4, 4), (1, 10, 0, 4),
                 (1, 10, lib.abn_hmm_max_k() + 1, 4), (1, 10, 4, 0), (1, 10, 4, lib.abn_gmm_max_d() + 1)):
        assert ws(*args) == -1, args
        assert b'abn_hmm_viterbi_ws_bytes' in lib.abn_last_error()


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    call = lib.abn_hmm_viterbi
    #       x  T    D  off len n  sh A  B  c0 lw ls lr K  ids lp nsw ng ws  bytes stream
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, p, p, 8, p, None, None, None, p, big, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 11, 12, 14):                    # every pointer but log_prob, n_switch, n_good
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG                 # T
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a13=0) == _lib.E_ARG    # D, n_utt, K
    assert with_(a2=lib.abn_gmm_max_d() + 1) == _lib.E_UNSUPPORTED and with_(a13=lib.abn_hmm_max_k() + 1) == _lib.E_UNSUPPORTED
    assert with_(a18=None) == _lib.E_WORKSPACE and with_(a19=1024) == _lib.E_WORKSPACE
    assert b'abn_hmm_viterbi_ws_bytes' in lib.abn_last_error()
    assert with_(a19=2 * 128 * 128 * 4) == _lib.E_WORKSPACE                              # the slabs alone: no frame fits
    assert with_(a18=ctypes.c_void_p(0x10004)) == _lib.E_ARG
