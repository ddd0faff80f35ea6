"""The HMM with a full transition matrix on the host: the numpy restatement (tests/hmm_dense_np.py) against enumeration of
all paths and against the sticky restatement, the identities of the expected counts, EM monotonicity on a planted cyclic
corpus, the floor, the Python layer's checks and files, the abny_ ledger of include/abnet3_hip_next.h, and the refusals
that need no launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import hmm_dense_np as dn  # noqa: E402
import hmm_np  # noqa: E402
from conftest import ROOT  # noqa: E402

HEADER = os.path.join(ROOT, 'include', 'abnet3_hip_next.h')


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def random_model(rng, K):
    init = rng.dirichlet(np.ones(K)).astype(np.float32)
    trans = rng.dirichlet(np.ones(K), size=K).astype(np.float32)
    return init, trans


# ---- the restatement -----------------------------------------------------------------------------------------------------
def test_restatement_equals_enumeration_of_all_paths():
    rng = np.random.default_rng(3)
    n = 0
    for K in (1, 2, 3):
        for L in (1, 2, 3, 5):
            for where in ('none', 'first', 'middle', 'last', 'all'):
                bad = np.zeros(L, dtype=bool)
                if where == 'first':
                    bad[0] = True
                elif where == 'middle':
                    bad[L // 2] = True
                elif where == 'last':
                    bad[-1] = True
                elif where == 'all':
                    bad[:] = True
                logn = rng.normal(size=(L, K)) * 3.0
                init, trans = random_model(rng, K)
                gamma, ll, xi, first = dn.brute_force(logn, bad, init, trans)
                for fb in (dn.forward_backward, dn.forward_backward_fast):
                    r = fb(logn, bad, init, trans)
                    assert np.abs(r['gamma'] - gamma).max() <= 1e-12, (K, L, where)
                    assert abs(r['loglik'] - ll) <= 1e-10 * (1.0 + abs(ll))
                    assert np.abs(r['xi'] - xi).max() <= 1e-12 and np.abs(r['first'] - first).max() <= 1e-12
                    assert r['n_good'] == int((~bad).sum()) and not r['gamma'][bad].any()
                f = dn.forward_backward(logn, bad, init, trans, smooth=False)
                assert not f['xi'].any() and not f['first'].any() and np.array_equal(f['gamma'], f['ahat'])
                r32 = dn.forward_backward(logn, bad, init, trans, np.float32)
                assert r32['gamma'].dtype == np.float32 and np.abs(r32['gamma'] - gamma).max() <= 1e-4
                n += 1
    assert n == 3 * 4 * 5


def test_sticky_matrix_gives_the_sticky_restatement_and_its_per_component_stays():
    rng = np.random.default_rng(4)
    for K, L, stay in ((2, 9, 0.5), (4, 30, 0.9), (7, 12, 0.0)):
        w = rng.dirichlet(np.full(K, 3.0))
        logn = rng.normal(size=(L, K)) * 2.0
        bad = rng.random(L) < 0.15
        init, trans = dn.sticky_matrix(w, stay)
        r = dn.forward_backward(logn, bad, init, trans)
        s = hmm_np.forward_backward(logn, bad, w.astype(np.float32), stay)
        assert np.abs(r['gamma'] - s['gamma']).max() <= 1e-7                    # (trans is rounded to float32 once)
        assert abs(r['loglik'] - s['loglik']) <= 1e-6 * L and r['n_good'] == s['n_good']
        # stay_k[k] = xi[k][k] stay / (stay + (1 - stay) w[k]): the share of "stayed" in the transition k -> k
        w32 = w.astype(np.float32).astype(np.float64)
        rho, omr = float(np.float32(stay)), float(np.float32(1.0) - np.float32(stay))
        stay_k = np.diag(r['xi']) * rho / (rho + omr * w32)
        assert abs(stay_k.sum() - s['stays']) <= 1e-6 * max(1, s['n_good'])


def test_identities_of_the_expected_counts():
    rng = np.random.default_rng(5)
    K = 4
    lens = np.array([1, 2, 7, 30, 5])
    off = np.cumsum(lens) - lens
    T = int(lens.sum())
    logn = rng.normal(size=(T, K)) * 2.0
    bad = rng.random(T) < 0.2
    bad[off[4]:off[4] + 5] = True                                              # an utterance that is all BAD
    init, trans = random_model(rng, K)
    for fast in (False, True):
        r = dn.corpus(logn, bad, off, lens, init, trans, fast=fast)
        assert abs(r['xi'].sum() - np.maximum(r['n_good'] - 1, 0).sum()) <= 1e-9
        but_last, but_first = np.zeros(K), np.zeros(K)
        for o, n in zip(off, lens):
            good = o + np.flatnonzero(~bad[o:o + n])
            but_last += r['post'][good[:-1]].sum(axis=0)
            but_first += r['post'][good[1:]].sum(axis=0)
        assert np.abs(r['xi'].sum(axis=1) - but_last).max() <= 1e-9
        assert np.abs(r['xi'].sum(axis=0) - but_first).max() <= 1e-9
        assert abs(r['first'].sum() - (r['n_good'] > 0).sum()) <= 1e-9


def test_em_does_not_decrease_the_penalised_likelihood_and_recovers_the_planted_cycle():
    import gmm_np
    x, lens, mu, _ = dn.planted_cycle(0)
    K = len(mu)
    off = np.cumsum(lens) - lens
    shift = np.zeros(x.shape[1], dtype=np.float32)
    xc, bad = gmm_np.centre(x, shift)
    A, B, _ = gmm_np.tables(np.full(K, 1.0 / K), mu, np.ones_like(mu))
    s64 = gmm_np.scores(xc, bad, A, B, hmm_np.emission_offsets(mu, np.ones_like(mu)), np.float64)
    utts = [(s64[o:o + n], bad[o:o + n]) for o, n in zip(off, lens)]
    for alpha in (0.0, 1e-3, 1.0):
        init0, trans0 = dn.sticky_matrix(np.full(K, 1.0 / K), 0.5)
        inits, transs, lls = dn.em(utts, init0, trans0, alpha, n_iter=8)
        obj = [ll + alpha * (np.log(t).sum() + np.log(i).sum()) for ll, t, i in zip(lls, transs, inits)]
        assert (np.diff(obj) >= -1e-7 * abs(obj[0])).all(), (alpha, np.diff(obj))
        t = transs[-1]
        for k in range(K):
            offd = t[k].copy()
            offd[k] = -1.0
            assert int(np.argmax(offd)) == (k + 1) % K, (alpha, t)
        if alpha < 1.0:
            assert np.abs(np.diag(t) - 0.8).max() <= 0.03 and np.abs(t[np.arange(K), (np.arange(K) + 1) % K] - 0.2).max() <= 0.03


def test_the_floor_keeps_every_entry_above_the_range_condition():
    from abnet3_amd import hmm
    assert hmm.TRANS_MIN == dn.TRANS_MIN == 2.0 ** -80 and hmm.TINY == dn.TINY == 2.0 ** -100
    K = 128
    stats = np.zeros((K + 1, K))
    stats[:K, 0] = 1e6                                                          # all the mass on one column, alpha = 0
    stats[3, :] = 0.0                                                           # a row without mass keeps its old values
    stats[K, 5] = 7.0
    old_t, old_i = np.full((K, K), 1.0 / K), np.full(K, 1.0 / K)
    for fn in (hmm.transition_update, lambda s, t, i, a: dn.mstep(s[:K], s[K], t, i, a)):
        t, i = fn(stats, old_t, old_i, 0.0)
        assert t.min() >= 2.0 ** -81 and i.min() >= 2.0 ** -81 and t.astype(np.float32).min() >= 2.0 ** -100
        assert np.abs(t.sum(axis=1) - 1.0).max() <= 1e-12 and abs(i.sum() - 1.0) <= 1e-12
        assert np.array_equal(t[3], old_t[3]) and abs(t[0, 0] - 1.0) <= 1e-12 and abs(i[5] - 1.0) <= 1e-12
        hmm.check_transitions('t', i, t)
    a, b = hmm.transition_update(stats, old_t, old_i, 0.5), dn.mstep(stats[:K], stats[K], old_t, old_i, 0.5)
    assert np.allclose(a[0], b[0], rtol=1e-14, atol=0) and np.allclose(a[1], b[1], rtol=1e-14, atol=0)
    assert abs(a[0][3, 0] - 1.0 / K) <= 1e-15                                   # alpha alone: uniform
    kept = hmm.transition_update(stats, old_t, old_i, 0.5, params='i')
    assert np.array_equal(kept[0], old_t) and not np.array_equal(kept[1], old_i)


def test_bigram_counts():
    from abnet3_amd import hmm
    ids = {'a': np.array([0, 0, 1, -1, 2, 2], dtype=np.int32), 'b': np.array([-1], dtype=np.int32), 'c': np.array([2, 0], dtype=np.int32),
           'd': np.zeros(0, dtype=np.int32)}
    want = np.zeros((3, 3), dtype=np.int64)
    for j, k in ((0, 0), (0, 1), (1, 2), (2, 2), (2, 0)):
        want[j, k] += 1
    for fn in (hmm.bigram_counts, dn.bigram_counts):
        got = fn(ids, 3)
        assert got.dtype == np.int64 and np.array_equal(got, want)
    with pytest.raises(ValueError, match='unit id'):
        hmm.bigram_counts(ids, 2)
    rng = np.random.default_rng(1)
    big = {str(i): rng.integers(-1, 6, size=50) for i in range(10)}
    assert np.array_equal(hmm.bigram_counts(big, 6), dn.bigram_counts(big, 6))


# ---- the Python layer ------------------------------------------------------------------------------------------------------
def test_python_layer_checks_and_files(lib, tmp_path):
    import abnet3_amd
    from abnet3_amd import hmm
    from abnet3_amd.gmm import GmmPosteriorgram
    from test_hmm_host import fitted_mixture
    assert abnet3_amd.TransitionHmmPosteriorgram is hmm.TransitionHmmPosteriorgram
    assert hmm.dense_max_k() >= 128
    g = fitted_mixture()
    h = hmm.TransitionHmmPosteriorgram(g, stay=0.75)
    i0, t0 = dn.sticky_matrix(g.weights_, 0.75)
    assert np.array_equal(h.init_, i0.astype(np.float64)) and np.array_equal(h.trans_, t0.astype(np.float64)) and h.alpha == 1e-3
    s = hmm.StickyHmmPosteriorgram(g, 0.6)
    f = hmm.TransitionHmmPosteriorgram.from_sticky(s)
    assert np.array_equal(f.trans_, dn.sticky_matrix(g.weights_, s.stay_)[1].astype(np.float64))
    dead = fitted_mixture()
    dead.weights_ = np.array([0.5, 0.0, 0.5])
    with pytest.raises(ValueError, match=r'\[1\]'):
        hmm.TransitionHmmPosteriorgram.from_sticky(hmm.StickyHmmPosteriorgram(dead, 0.6))
    with pytest.raises(ValueError, match=r'\[1\]'):
        hmm.TransitionHmmPosteriorgram(dead)
    # the range and the shape of init / trans
    good_t = np.full((3, 3), 1.0 / 3)
    for bad_t in (np.array([[1.0, 0.0, 0.0]] * 3), np.full((3, 3), 0.5), np.full((2, 2), 0.5), np.full((3, 3), np.nan)):
        with pytest.raises(ValueError):
            hmm.TransitionHmmPosteriorgram(g, trans=bad_t)
    tiny = good_t.copy()
    tiny[0] = [1.0 - 2.0 ** -101, 2.0 ** -102, 2.0 ** -102]
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.TransitionHmmPosteriorgram(g, trans=tiny)
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.TransitionHmmPosteriorgram(g, trans=good_t, init=[1.0, 0.0, 0.0])
    with pytest.raises(ValueError, match='alpha'):
        hmm.TransitionHmmPosteriorgram(g, alpha=-1.0)
    with pytest.raises(ValueError, match='fitted'):
        hmm.TransitionHmmPosteriorgram(GmmPosteriorgram(3))
    for params in ('', 'mm', 'w', 'mvs', None):
        with pytest.raises(ValueError, match='params'):
            h.fit(torch.zeros(5, 2), params=params)
    # the table-level call refuses on the host, before any device is needed
    z = lambda *s: torch.zeros(*s)
    it, tt = torch.from_numpy(i0), torch.from_numpy(t0)
    with pytest.raises(ValueError, match='mode'):
        hmm.dense_forward_backward(z(6, 2), [0], [6], z(2), z(3, 2), z(3, 2), z(3), it, tt, mode='both')
    with pytest.raises(ValueError, match='init'):
        hmm.dense_forward_backward(z(6, 2), [0], [6], z(2), z(3, 2), z(3, 2), z(3), it[:2], tt)
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.dense_forward_backward(z(6, 2), [0], [6], z(2), z(3, 2), z(3, 2), z(3), it, torch.eye(3))
    with pytest.raises(ValueError, match='overlap'):
        hmm.dense_forward_backward(z(6, 2), [0, 2], [4, 4], z(2), z(3, 2), z(3, 2), z(3), it, tt)
    with pytest.raises(ValueError, match='outside'):
        hmm.dense_forward_backward(z(6, 2), [0], [7], z(2), z(3, 2), z(3, 2), z(3), it, tt)
    K = hmm.dense_max_k() + 1
    with pytest.raises(ValueError, match='abny_hmm_dense_max_k'):
        hmm.dense_forward_backward(z(6, 2), [0], [6], z(2), z(K, 2), z(K, 2), z(K), torch.full((K,), 1.0 / K), torch.full((K, K), 1.0 / K))
    # save / load
    h.trans_ = dn.floor_rows(np.random.default_rng(0).dirichlet(np.ones(3), size=3))
    h.init_ = np.array([0.2, 0.3, 0.5])
    h.log_likelihoods = [-3.0, -2.5]
    path = str(tmp_path / 'dense.npz')
    h.save(path)
    b = hmm.TransitionHmmPosteriorgram.load(path)
    assert np.array_equal(b.trans_, h.trans_) and np.array_equal(b.init_, h.init_) and b.alpha == h.alpha
    assert b.log_likelihoods == h.log_likelihoods and np.array_equal(b.gmm.means_, g.means_)
    assert np.array_equal(GmmPosteriorgram.load(path).means_, g.means_)          # the mixture's reader still reads it
    gpath = str(tmp_path / 'gmm.npz')
    g.save(gpath)
    with pytest.raises(ValueError, match='no trans'):
        hmm.TransitionHmmPosteriorgram.load(gpath)
    assert b.whoami()['class_name'] == 'TransitionHmmPosteriorgram'
    text = open(os.path.join(ROOT, 'abnet3_amd', 'hmm.py')).read() + open(os.path.join(ROOT, 'examples', 'zero_resource.py')).read()
    assert "'fit-trans'" in text and "'--hmm-trans'" in text


# ---- the library -----------------------------------------------------------------------------------------------------------
def declared():
    text = re.sub(r'/\*.*?\*/', '', open(HEADER).read(), flags=re.S)
    return set(re.findall(r'\b(abny_[a-z0-9_]+)\s*\(', text))


def test_next2_symbols_are_the_headers_second_section_and_the_librarys_exports(lib):
    import subprocess
    from abnet3_amd import _lib
    assert declared() == set(_lib.NEXT2_SYMBOLS) == {'abny_hmm_dense_max_k', 'abny_hmm_dense_ws_bytes', 'abny_hmm_dense_forward_backward'}
    assert not set(_lib.NEXT2_SYMBOLS) & set(_lib.SYMBOLS) and not set(_lib.NEXT2_SYMBOLS) & set(_lib.NEXT_SYMBOLS)
    assert not set(_lib.NEXT_SYMBOLS) & set(_lib.SYMBOLS)
    nm = '/opt/rocm/lib/llvm/bin/llvm-nm' if os.path.exists('/opt/rocm/lib/llvm/bin/llvm-nm') else 'nm'
    out = subprocess.run([nm, '-D', '--defined-only', lib._name], stdout=subprocess.PIPE, text=True, check=True).stdout
    exported = {p[2] for p in (line.split() for line in out.splitlines()) if len(p) >= 3 and p[1] in 'TtWw' and p[2].startswith('abny_')}
    assert exported == declared()
    for name, (res, args) in _lib.NEXT2_SYMBOLS.items():
        fn = getattr(lib, name)
        assert fn.restype is res and list(fn.argtypes) == list(args)
    assert lib.abny_hmm_dense_max_k() >= 128
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20                     # not part of the numbered ABI yet


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    #       x  T    D  off len n  sh A  B  c0 init trans K mode post ll ng stats ws bytes stream
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, p, 8, 0, p, p, p, None, p, big, None]
    call = lib.abny_hmm_dense_forward_backward
    name = b'abny_hmm_dense_forward_backward'

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 11, 14, 15, 16):
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error() and name in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a12=0) == _lib.E_ARG
    for mode in (-1, 2, 3):
        assert with_(a13=mode) == _lib.E_ARG and b'mode' in lib.abn_last_error()
    max_k, max_d = lib.abny_hmm_dense_max_k(), lib.abn_gmm_max_d()
    assert with_(a12=max_k + 1) == _lib.E_UNSUPPORTED and b'abny_hmm_dense_max_k' in lib.abn_last_error()
    assert with_(a2=max_d + 1) == _lib.E_UNSUPPORTED and b'abn_gmm_max_d' in lib.abn_last_error()
    assert with_(a18=None) == _lib.E_WORKSPACE and with_(a19=1024) == _lib.E_WORKSPACE
    assert b'abny_hmm_dense_ws_bytes' in lib.abn_last_error()
    assert with_(a19=lib.abny_hmm_dense_ws_bytes(2, 1, 8, 4) - 256 * 2) == _lib.E_WORKSPACE    # (one frame short in both regions)
    assert with_(a18=ctypes.c_void_p(0x10004)) == _lib.E_ARG
    # the sizing entry
    ws = lib.abny_hmm_dense_ws_bytes
    assert ws(2, 100, 8, 4) > 0 and ws(2, 100, 8, 4) % 256 == 0 and ws(2, 101, 128, 4) > ws(2, 100, 128, 4) - 1
    assert ws(300, 10, 8, 4) == ws(256, 10, 8, 4)                                      # min(n_utt, 256) workgroups
    # the slab of scores, the float64 statistics of the capacity K rounds up to, and c_t per frame, rounded up to 256
    up = lambda v: (v + 255) // 256 * 256
    assert ws(1, 64, 128, 4) == up(128 * 128 * 4 + 8 * (128 * 128 + 128) + 64 * 4)
    assert ws(1, 64, 5, 4) == up(128 * 128 * 4 + 8 * (16 * 16 + 16) + 64 * 4)
    for bad in ((0, 10, 8, 4), (2, -1, 8, 4), (2, lib.abn_hmm_max_len() + 1, 8, 4), (2, 10, 0, 4), (2, 10, max_k + 1, 4),
                (2, 10, 8, 0), (2, 10, 8, max_d + 1)):
        assert ws(*bad) == -1 and b'abny_hmm_dense_ws_bytes' in lib.abn_last_error(), bad
