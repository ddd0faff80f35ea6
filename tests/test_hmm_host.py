"""The sticky HMM of abnet3_amd/hmm.py on the host: the numpy restatement (tests/hmm_np.py) against enumeration of all
paths, its special cases, EM on the stay probability, and everything the library and the Python layer refuse before a
launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_hmm_forward_backward', 'abn_hmm_ws_bytes', 'abn_hmm_max_len', 'abn_hmm_max_k')
RHOS = (0.0, 0.5, 0.9)


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def small_cases():
    """K = 1 .. 3, up to 6 frames, with and without a BAD frame."""
    rng = np.random.default_rng(3)
    out = []
    for K in (1, 2, 3):
        for L in (1, 2, 3, 6):
            for with_bad in (False, True):
                logn = rng.normal(size=(L, K)) * 3.0
                bad = np.zeros(L, dtype=bool)
                if with_bad:
                    bad[rng.integers(0, L)] = True
                    if L == 6:
                        bad[0] = True                                  # a leading BAD frame as well
                w = rng.dirichlet(np.ones(K)).astype(np.float32)
                out.append((logn, bad, w))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rho', RHOS)
def test_restatement_agrees_with_the_enumeration_of_all_paths(rho):
    for logn, bad, w in small_cases():
        r = hmm_np.forward_backward(logn, bad, w, rho)
        gamma, ll, stays = hmm_np.brute_force(logn, bad, w, rho)
        assert np.abs(r['gamma'] - gamma).max() <= 1e-12
        assert abs(r['loglik'] - ll) <= 1e-12 * max(1.0, abs(ll))
        assert abs(r['stays'] - stays) <= 1e-12
        assert r['n_good'] == int((~bad).sum()) and not r['gamma'][bad].any()
        fast = hmm_np.forward_backward_fast(logn, bad, w, rho)
        assert abs(fast[0] - r['loglik']) <= 1e-12 * max(1.0, abs(ll)) and abs(fast[1] - r['stays']) <= 1e-12
        assert np.abs(fast[3] - r['gamma']).max() <= 1e-12 and np.abs(fast[4] - r['ahat']).max() <= 1e-12
        # the float32 forms of both agree to float32 rounding (they differ in the order of the sums over k only)
        r32, f32 = hmm_np.forward_backward(logn, bad, w, rho, np.float32), hmm_np.forward_backward_fast(logn, bad, w, rho, True, np.float32)
        assert r32['gamma'].dtype == np.float32 and f32[3].dtype == np.float32
        assert np.abs(f32[3] - r32['gamma']).max() <= 1e-5 and np.abs(r32['gamma'] - gamma).max() <= 1e-5


def test_zero_stay_is_the_frame_independent_mixture():
    rng = np.random.default_rng(5)
    T, K, D = 40, 7, 5
    x = rng.normal(size=(T, D)).astype(np.float32) * 2.0
    x[11, 2] = np.nan
    w = rng.dirichlet(np.ones(K))
    m, v = rng.normal(size=(K, D)), rng.uniform(0.5, 2.0, size=(K, D))
    xc, bad = gmm_np.centre(x, np.zeros(D, dtype=np.float32))
    A, B, c = gmm_np.tables(w, m, v)
    lse, g = gmm_np.lse_post(gmm_np.scores(xc, bad, A, B, c), bad)
    c0 = hmm_np.emission_offsets(m, v)
    r = hmm_np.forward_backward(gmm_np.scores(xc, bad, A, B, c0), bad, w.astype(np.float32), 0.0)
    # (c and c0 + log w32 differ by the roundings of c, c0 and w to float32: a few 2^-24 of their size)
    tol = 8 * 2.0 ** -24 * (np.abs(c).max() + 1.0)
    assert np.abs(r['gamma'] - g).max() <= tol
    assert abs(r['loglik'] - lse[~bad].sum()) <= tol * (~bad).sum()
    assert r['stays'] == 0.0 and not r['gamma'][11].any()
    assert np.abs(r['gamma'] - r['ahat']).max() <= 1e-14              # bhat = sum_k w bt / c = 1 up to rounding


@pytest.mark.parametrize('dtype', [np.float64, np.float32])
def test_rows_sum_to_one(dtype):
    rng = np.random.default_rng(6)
    logn = rng.normal(size=(30, 5)) * 10.0
    bad = rng.random(30) < 0.2
    w = rng.dirichlet(np.ones(5)).astype(np.float32)
    w[3] = 0.0                                                        # a component of weight 0 keeps gamma = 0
    for rho in (0.0, 0.5, 0.9, 0.999):
        for smooth in (True, False):
            r = hmm_np.forward_backward(logn, bad, w, rho, dtype, smooth)
            sums = r['gamma'].astype(np.float64).sum(axis=1)
            assert np.abs(sums[~bad] - 1.0).max() <= (1e-12 if dtype is np.float64 else 1e-5)
            assert not r['gamma'][bad].any() and not r['gamma'][:, 3].any()


def planted_utterances(seed):
    x, lens, w, mu = hmm_np.planted(seed)
    logn = -0.5 * ((x.astype(np.float64)[:, None, :] - mu[None]) ** 2).sum(axis=2)
    bad = np.zeros(len(x), dtype=bool)
    off = np.cumsum(lens) - lens
    return [(logn[o:o + n], bad[o:o + n]) for o, n in zip(off, lens)], w.astype(np.float32)


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_em_is_monotone_and_recovers_a_planted_stay(seed):
    utts, w32 = planted_utterances(seed)
    rhos, lls = hmm_np.em_stay(utts, w32, 0.5, n_iter=10)
    print('seed %d: stay %s' % (seed, ' '.join('%.4f' % r for r in rhos)))
    # float64 EM never lowers the likelihood (slack: the rounding of a sum of 10,000 terms of size ~10, and of rho to fp32)
    assert (np.diff(lls) >= -1e-6 * abs(lls[-1])).all(), np.diff(lls)
    assert abs(rhos[-1] - 0.9) <= 0.02, rhos


# ---- the library -------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_names(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20


def test_sizing_queries_and_refusals(lib):
    from abnet3_amd import hmm
    ws = lib.abn_hmm_ws_bytes
    assert hmm.max_k() == lib.abn_hmm_max_k() == lib.abn_gmm_max_k()
    assert hmm.max_len() == lib.abn_hmm_max_len() >= 1 << 16
    up = lambda v: (v + 255) // 256 * 256
    # per workgroup (one per utterance, 256 at most): 128 x (K rounded up to 128) fp32 scores and one float per frame
    layout = lambda n_utt, max_len, K: min(n_utt, 256) * up(128 * ((K + 127) // 128 * 128) * 4 + 4 * max_len)
    for n_utt, max_len, K, D in ((1, 1, 1, 1), (3, 300, 129, 40), (5000, 1000, 1024, 100), (256, 0, 300, 8), (257, 130, 4096, 127)):
        assert ws(n_utt, max_len, K, D) == layout(n_utt, max_len, K), (n_utt, max_len, K, D)
    # no T x K array beyond the output: 1.14 M frames in utterances of up to 1000 frames, K = 1024
    assert ws(2000, 1000, 1024, 40) < 1140000 * 1024 * 4 // 8
    for args in ((0, 10, 4, 4), (1 << 31, 10, 4, 4), (1, -1, 4, 4), (1, lib.abn_hmm_max_len() + 1, 4, 4), (1, 10, 0, 4),
                 (1, 10, lib.abn_hmm_max_k() + 1, 4), (1, 10, 4, 0), (1, 10, 4, lib.abn_gmm_max_d() + 1)):
        assert ws(*args) == -1, args
        assert b'abn_hmm_ws_bytes' in lib.abn_last_error()


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    call = lib.abn_hmm_forward_backward
    #       x  T    D  off len n  sh A  B  c0 w  K  rho  mode post ll stays ng ws  bytes stream
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, 8, 0.5, 0, p, p, None, p, p, big, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 14, 15, 17):                    # every pointer but stays
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG                 # T
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a11=0) == _lib.E_ARG    # D, n_utt, K
    assert with_(a2=lib.abn_gmm_max_d() + 1) == _lib.E_UNSUPPORTED and with_(a11=lib.abn_hmm_max_k() + 1) == _lib.E_UNSUPPORTED
    for rho in (-0.5, 1.0, 1.5, float('nan'), float('inf')):
        assert with_(a12=rho) == _lib.E_ARG
        assert b'rho' in lib.abn_last_error()
    assert with_(a13=2) == _lib.E_ARG and with_(a13=-1) == _lib.E_ARG
    assert with_(a18=None) == _lib.E_WORKSPACE and with_(a19=1024) == _lib.E_WORKSPACE
    assert with_(a19=2 * 128 * 128 * 4) == _lib.E_WORKSPACE                              # the slabs alone: no frame fits
    assert with_(a18=ctypes.c_void_p(0x10004)) == _lib.E_ARG


def fitted_mixture(K=3, D=2):
    from abnet3_amd.gmm import GmmPosteriorgram
    g = GmmPosteriorgram(K)
    g.weights_ = np.full(K, 1.0 / K)
    g.means_, g.variances_ = np.arange(K * D, dtype=np.float64).reshape(K, D), np.ones((K, D))
    g.shift_, g.gv_ = np.zeros(D, dtype=np.float32), np.ones(D)
    return g


def test_python_layer_refuses_on_the_host(lib, tmp_path):
    import abnet3_amd
    from abnet3_amd import hmm
    from abnet3_amd.gmm import GmmPosteriorgram
    assert abnet3_amd.StickyHmmPosteriorgram is hmm.StickyHmmPosteriorgram
    for bad in (-0.1, 1.0, 1.5, float('nan'), float('inf'), 'x', None):
        with pytest.raises(ValueError, match='stay'):
            hmm.check_stay('t', bad)
    assert hmm.check_stay('t', 0) == 0.0 and hmm.check_stay('t', 0.9) == float(np.float32(0.9))
    w = np.array([0.5, 0.5, 0.0], dtype=np.float32)
    assert hmm.check_stay('t', 0.9999, w) == float(np.float32(0.9999))                   # a zero weight does not count
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.check_stay('t', 0.5, np.array([1.0, 2.0 ** -100], dtype=np.float32))
    assert hmm.check_stay('t', 0.5, np.array([1.0, 2.0 ** -99], dtype=np.float32)) == 0.5
    with pytest.raises(ValueError, match='weights'):
        hmm.check_stay('t', 0.5, np.zeros(3, dtype=np.float32))
    with pytest.raises(ValueError, match='fitted'):
        hmm.StickyHmmPosteriorgram(GmmPosteriorgram(3))
    with pytest.raises(ValueError, match='stay'):
        hmm.StickyHmmPosteriorgram(fitted_mixture(), 1.0)
    h = hmm.StickyHmmPosteriorgram(fitted_mixture(), 0.75)
    assert h.stay_ == 0.75
    with pytest.raises(ValueError, match='D = 4'):
        h.transform(torch.zeros(5, 4))
    with pytest.raises(ValueError, match='float32'):
        h.transform(torch.zeros(5, 2, dtype=torch.float64))
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    args = lambda **kw: dict(dict(table=z(6, D), off=[0, 3], lens=[3, 3], shift=z(D), A=z(K, D), B=z(K, D), c0=z(K),
                                  w=torch.full((K,), 1.0 / K), stay=0.5), **kw)
    for kw, match in ((dict(mode='viterbi'), 'mode'), (dict(table=z(6, D).double()), 'float32'), (dict(A=z(K, D + 1)), 'A \\[K, D\\]'),
                      (dict(stay=1.0), 'stay'), (dict(w=z(K)), 'weights'), (dict(lens=[3]), 'offsets'),
                      (dict(lens=[3, 4]), 'outside'), (dict(off=[-1, 3]), 'outside'), (dict(off=[0, 2]), 'overlap'),
                      (dict(table=z(hmm.max_len() + 1, D), off=[0], lens=[hmm.max_len() + 1]), 'abn_hmm_max_len')):
        with pytest.raises(ValueError, match=match):
            hmm.forward_backward(**args(**kw))
    # save / load keep the mixture and the stay
    path = str(tmp_path / 'hmm.npz')
    h.log_likelihoods = [-3.0, -2.5]
    h.save(path)
    h2 = hmm.StickyHmmPosteriorgram.load(path)
    assert h2.stay_ == 0.75 and h2.log_likelihoods == [-3.0, -2.5]
    assert np.array_equal(h2.gmm.means_, h.gmm.means_) and np.array_equal(h2.gmm.weights_, h.gmm.weights_)
    assert GmmPosteriorgram.load(path).n_components == 3                                  # still a mixture file
    gpath = str(tmp_path / 'gmm.npz')
    h.gmm.save(gpath)
    with pytest.raises(ValueError, match='no stay'):
        hmm.StickyHmmPosteriorgram.load(gpath)


def test_emission_offsets_are_c_without_the_log_weight():
    from abnet3_amd import gmm, hmm
    rng = np.random.default_rng(8)
    w, m, v = rng.dirichlet(np.ones(6)), rng.normal(size=(6, 4)), rng.uniform(0.5, 2.0, size=(6, 4))
    w[2] = 0.0
    c0 = hmm.emission_offsets(m, v)
    assert np.array_equal(c0, hmm_np.emission_offsets(m, v)) and np.isfinite(c0).all()
    _, _, c = gmm.score_tables(w, m, v)
    live = w > 0
    assert np.abs(c0[live].astype(np.float64) + np.log(w[live]) - c[live]).max() <= 2.0 ** -22 * np.abs(c).max()
