"""Baum-Welch training of the sticky HMM on the host: the numpy restatement (tests/hmm_bw_np.py) against enumeration of
all paths and all switch sequences, float64 EM on planted corpora, the host M-step of abnet3_amd/hmm.py, and everything
the library and the Python layer refuse before a launch.  No kernel runs here."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import gmm_np  # noqa: E402
import hmm_bw_np  # noqa: E402
import hmm_np  # noqa: E402
from conftest import ROOT  # noqa: E402

NAMES = ('abn_hmm_forward_backward_stats', 'abn_hmm_accumulate_ws_bytes', 'abn_hmm_accumulate')
RHOS = (0.0, 0.5, 0.9)


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def small_cases():
    """K = 2, 3; up to 5 good frames; no BAD frame, one in the middle, one as the first frame; a weight-0 component."""
    rng = np.random.default_rng(11)
    out = []
    for K in (2, 3):
        for L, bad_at in ((1, None), (2, None), (4, None), (5, None), (5, 2), (6, 3), (5, 0), (6, 0)):
            for zero_weight in (False, True):
                logn = rng.normal(size=(L, K)) * 3.0
                bad = np.zeros(L, dtype=bool)
                if bad_at is not None:
                    bad[bad_at] = True
                w = rng.dirichlet(np.ones(K))
                if zero_weight:
                    w[K - 1] = 0.0
                    w /= w.sum()
                out.append((logn, bad, w.astype(np.float32)))
    return out


# ---- the restatement ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize('rho', RHOS)
def test_stays_and_draws_agree_with_the_enumeration_of_paths_and_switches(rho):
    for logn, bad, w in small_cases():
        r = hmm_bw_np.forward_backward(logn, bad, w, rho)
        sk, dr = hmm_bw_np.brute_force(logn, bad, w, rho)
        assert (~bad).sum() <= 5
        assert np.abs(r['stay_k'] - sk).max() <= 1e-12 and np.abs(r['draws'] - dr).max() <= 1e-12
        assert not r['stay_k'][w == 0].any() and not r['draws'][w == 0].any()
        # the recursion is hmm_np's: gamma, loglik and the scalar stays
        ref = hmm_np.forward_backward(logn, bad, w, rho)
        assert np.abs(r['gamma'] - ref['gamma']).max() <= 1e-12 and abs(r['loglik'] - ref['loglik']) <= 1e-12 * max(1.0, abs(ref['loglik']))
        assert abs(r['stays'] - ref['stays']) <= 1e-12 and r['n_good'] == ref['n_good']
        # sum_k stay_k == stays and sum_k draws == n_good - stays
        assert abs(r['stay_k'].sum() - r['stays']) <= 1e-12
        assert abs(r['draws'].sum() - (r['n_good'] - r['stays'])) <= 1e-12
        if rho == 0.0:
            assert not r['stay_k'].any()


def planted_start(seed):
    """hmm_np.planted(seed, 60 utterances of 50 frames) and gmm.py's start: K random rows, the global variance, uniform weights."""
    x, lens, _, _ = hmm_np.planted(seed, n_utt=60, L=50)
    shift, gv = gmm_np.moments(x)
    xc, bad = gmm_np.centre(x, shift)
    w, m, v = gmm_np.initial(xc, bad, gv, 4, seed)
    return xc, bad, np.cumsum(lens) - lens, lens, gv, w, m, v


@pytest.fixture(scope='module')
def planted():
    cache = {}

    def get(seed):
        if seed not in cache:
            cache[seed] = planted_start(seed)
        return cache[seed]
    return get


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_float64_em_never_lowers_the_likelihood(planted, seed):
    xc, bad, off, lens, gv, w, m, v = planted(seed)
    n = float(lens.sum())
    for params in ('mvws', 'mv', 'w', 'ms', 'v'):
        r = hmm_bw_np.em(xc, bad, off, lens, w, m, v, 0.5, gv, n_iter=12 if params == 'mvws' else 5, params=params)
        lls = np.array(r['log_likelihoods'])
        print('seed %d params %s: per-frame log-likelihood %.4f -> %.4f, stay %.4f' % (seed, params, lls[0], lls[-1], r['rho']))
        assert (np.diff(lls) >= -1e-9).all(), (params, np.diff(lls))
        assert abs(r['w'].sum() - 1.0) <= 1e-12 and (r['v'] > 0).all()
        if params == 'mv':                                              # the weights and the stay do not move
            assert np.array_equal(r['w'], w) and r['rhos'] == [0.5] * len(r['rhos'])
        if params == 'mvws':
            assert lls[-1] - lls[0] > 0.5 and len(lls) == 12
    assert n == 3000.0


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_the_stay_alone_reproduces_em_stay(planted, seed):
    xc, bad, off, lens, gv, w, m, v = planted(seed)
    r = hmm_bw_np.em(xc, bad, off, lens, w, m, v, 0.5, gv, n_iter=6, params='s', stay_from_stays=True)
    s = hmm_bw_np.e_step(xc, bad, off, lens, w, m, v, 0.5)['scores']
    rhos, lls = hmm_np.em_stay([(s[o:o + n], bad[o:o + n]) for o, n in zip(off, lens)], w.astype(np.float32), 0.5, n_iter=6)
    assert r['rhos'] == rhos and r['totals'] == lls
    assert np.array_equal(r['w'], w) and np.array_equal(r['m'], m) and np.array_equal(r['v'], v)
    # the stay from sum_k stay_k is the same number up to the rounding of a float64 sum, then rounded to float32
    r2 = hmm_bw_np.em(xc, bad, off, lens, w, m, v, 0.5, gv, n_iter=6, params='s')
    assert np.abs(np.array(r2['rhos']) - np.array(rhos)).max() <= 2.0 ** -23


# ---- the host M-step ---------------------------------------------------------------------------------------------------
def hand_made():
    K, D = 4, 2
    m = np.array([[0.0, 1.0], [2.0, -1.0], [5.0, 5.0], [-3.0, 0.5]])
    v = np.array([[1.0, 2.0], [0.5, 0.5], [3.0, 3.0], [1.0, 1.0]])
    gv = np.array([4.0, 9.0])
    N = np.array([10.0, 20.0, 0.25, 8.0])                              # component 2 is starved (min_count 1)
    mean = np.array([[0.5, 1.5], [2.5, -0.5], [9.0, 9.0], [-2.0, 0.0]])
    var = np.array([[2.0, 1.0], [1e-4, 3.0], [1.0, 1.0], [0.7, 1e-9]])   # two entries below the floor 0.01 gv = (0.04, 0.09)
    sums = np.concatenate([N[:, None] * mean, N[:, None] * (var + mean * mean), N[:, None]], axis=1)
    sk = np.array([6.0, 15.0, 0.05, 7.5])
    return K, D, m, v, gv, N, mean, var, sums, sk


def test_baum_welch_update_on_hand_made_sums():
    from abnet3_amd import hmm
    K, D, m, v, gv, N, mean, var, sums, sk = hand_made()
    w0 = np.full(K, 0.25)
    w, m1, v1, stay, nret = hmm.baum_welch_update(sums, sk, 30, m, v, gv, 0.01, 1.0, 'mvws')
    ref = hmm_bw_np.m_step(sums, sk, 30, w0, m, v, 0.5, gv, 0.01, 1.0, 'mvws')
    for a, b in zip((w, m1, v1), ref[:3]):
        assert np.abs(a - b).max() <= 1e-15
    assert stay == ref[3] == float(np.float32(sk.sum() / 30)) and nret == ref[4] == 0
    # a starved component keeps its mean and variance; the others move to S1 / N and the floored second moment
    assert np.array_equal(m1[2], m[2]) and np.array_equal(v1[2], v[2])
    keep = [0, 1, 3]
    assert np.abs(m1[keep] - mean[keep]).max() <= 1e-14
    assert v1[1, 0] == 0.01 * gv[0] and v1[3, 1] == 0.01 * gv[1]          # the variance floor binds
    assert abs(v1[0, 0] - 2.0) <= 1e-13 and abs(v1[1, 1] - 3.0) <= 1e-13
    draws = N - sk
    assert np.abs(w - draws / draws.sum()).max() <= 1e-15 and abs(w.sum() - 1.0) <= 1e-15
    # the inputs are not written
    assert m[0, 0] == 0.0 and v[1, 0] == 0.5
    # held fixed: what is not named comes back as given
    w2, m2, v2, stay2, _ = hmm.baum_welch_update(sums, sk, 30, m, v, gv, 0.01, 1.0, 'v', weights=w0, stay=0.75)
    assert np.array_equal(w2, w0) and np.array_equal(m2, m) and stay2 == 0.75
    second = var + (mean - m) ** 2                                        # about the mean in force
    assert np.abs(v2[keep] - np.maximum(second, 0.01 * gv)[keep]).max() <= 1e-12 and np.array_equal(v2[2], v[2])
    w3, m3, v3, stay3, _ = hmm.baum_welch_update(sums, sk, 30, m, v, gv, 0.01, 1.0, 's', weights=w0, stay=0.1, stays_total=12.0)
    assert stay3 == float(np.float32(12.0 / 30)) and np.array_equal(m3, m) and np.array_equal(v3, v) and np.array_equal(w3, w0)
    assert hmm.baum_welch_update(sums, sk * 10.0, 30, m, v, gv, params='s', weights=w0)[3] == float(np.float32(hmm.STAY_MAX))
    for kw, match in ((dict(params='w'), 'stay'), (dict(params='s'), 'weights'), (dict(params='mvx'), 'params'), (dict(params=''), 'params'),
                      (dict(params='mm'), 'params'), (dict(params=None), 'params')):
        with pytest.raises(ValueError, match=match):
            hmm.baum_welch_update(sums, sk, 30, m, v, gv, **kw)
    with pytest.raises(ValueError, match='two good frames'):
        hmm.baum_welch_update(sums, sk, 0, m, v, gv, params='s', weights=w0)
    with pytest.raises(ValueError, match='sums'):
        hmm.baum_welch_update(sums[:, :-1], sk, 30, m, v, gv)


def test_a_weight_below_weight_min_is_retired_and_the_result_passes_check_stay():
    from abnet3_amd import hmm
    K, D, m, v, gv, N, mean, var, sums, sk = hand_made()
    assert hmm.WEIGHT_MIN == 2.0 ** -80 == hmm_bw_np.WEIGHT_MIN
    sums = sums.copy()
    sums[3, 2 * D] = 7.5 + 1e-30                                          # draws of 1e-30 in 23.2: a weight of 4e-32 < 2^-80
    w, _, _, stay, nret = hmm.baum_welch_update(sums, sk, 30, m, v, gv, 0.01, 1.0, 'ws')
    assert w[3] == 0.0 and nret == 1 and abs(w.sum() - 1.0) <= 1e-15 and (w[:3] > 0).all()
    assert hmm.check_stay('t', stay, w.astype(np.float32)) == stay       # the range condition cannot fail
    ref = hmm_bw_np.m_step(sums, sk, 30, np.full(K, 0.25), m, v, 0.5, gv, 0.01, 1.0, 'ws')
    assert np.abs(w - ref[0]).max() <= 1e-15 and ref[4] == 1
    # without the retirement the same weight is refused by the range condition at the largest stay
    with pytest.raises(ValueError, match='2\\^-100'):
        hmm.check_stay('t', hmm.STAY_MAX, np.array([1.0, 2.0 ** -90], dtype=np.float32))
    assert hmm.check_stay('t', hmm.STAY_MAX, np.array([1.0, hmm.WEIGHT_MIN], dtype=np.float32)) == float(np.float32(hmm.STAY_MAX))
    # rounding can leave N - stay_k a hair below 0: the draws are clamped, the weight is 0, the component retired
    sk2 = sk.copy()
    sk2[0] = 10.0 + 1e-12
    w2 = hmm.baum_welch_update(sums, sk2, 30, m, v, gv, params='w', stay=0.5)[0]
    assert w2[0] == 0.0 and (w2 >= 0).all() and abs(w2.sum() - 1.0) <= 1e-15
    # a retired component stays retired: its gamma is 0, so N = stay_k = 0 and its draws are 0
    sums3, sk3 = sums.copy(), sk.copy()
    sums3[1], sk3[1] = 0.0, 0.0
    w3, m3, v3, _, nret3 = hmm.baum_welch_update(sums3, sk3, 30, m, v, gv, params='mvws')
    assert w3[1] == 0.0 and nret3 == 2 and np.array_equal(m3[1], m[1]) and np.array_equal(v3[1], v[1])
    with pytest.raises(ValueError, match='draws'):
        hmm.baum_welch_update(sums, N, 30, m, v, gv, params='w', stay=0.5)


# ---- the library -------------------------------------------------------------------------------------------------------
def test_header_and_binding_carry_the_new_names(lib):
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    declared = set(re.findall(r'\b(abn_[a-z0-9_]+)\s*\(', text))
    for name in NAMES:
        assert name in declared and name in _lib.SYMBOLS and hasattr(lib, name), name
    assert _lib.ABI_VERSION == 20 and lib.abn_abi_version() == 20


def test_accumulate_sizing_and_refusals_before_any_launch(lib):
    from abnet3_amd import _lib
    ws = lib.abn_hmm_accumulate_ws_bytes
    # one fp32 slab [128][2D + 1] per (component tile, range): abn_gmm_accumulate's workspace
    for T, K, D, nr in ((1, 1, 1, 0), (1000, 130, 5, 3), (1000, 300, 40, 1), (1140000, 1024, 40, 0), (129, 4096, 127, 256)):
        assert ws(T, K, D, nr) == lib.abn_gmm_ws_bytes(T, K, D, nr) > 0, (T, K, D, nr)
    assert ws(1000, 130, 5, 3) == 2 * 3 * 128 * 11 * 4
    max_k, max_d = lib.abn_hmm_max_k(), lib.abn_gmm_max_d()
    for args in ((0, 4, 4, 0), (10, 0, 4, 0), (10, 4, 0, 0), (10, 4, 4, -1), (10, 4, 4, 257), (10, max_k + 1, 4, 0), (10, 4, max_d + 1, 0),
                 ((1 << 31) - 128, 4, 4, 0)):
        assert ws(*args) == -1, args
        assert b'abn_hmm_accumulate_ws_bytes' in lib.abn_last_error()
    p = ctypes.c_void_p(0x10000)
    big = 1 << 40
    #       x  T    D  shift post K  n_ranges sums ws bytes stream
    good = [p, 100, 4, p, p, 8, 0, p, p, big, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return lib.abn_hmm_accumulate(*a)
    for i in (0, 3, 4, 7):
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG      # T, D, K
    assert with_(a6=-1) == _lib.E_ARG and with_(a6=257) == _lib.E_ARG
    assert with_(a5=max_k + 1) == _lib.E_UNSUPPORTED and with_(a2=max_d + 1) == _lib.E_UNSUPPORTED
    assert with_(a1=(1 << 31) - 128) == _lib.E_UNSUPPORTED
    assert b'abn_hmm_accumulate' in lib.abn_last_error()
    need = ws(100, 8, 4, 0)
    assert with_(a8=None) == _lib.E_WORKSPACE and with_(a9=need - 1) == _lib.E_WORKSPACE and with_(a9=0) == _lib.E_WORKSPACE
    assert b'abn_hmm_accumulate_ws_bytes' in lib.abn_last_error()


def test_stats_entry_refuses_what_the_plain_entry_refuses_and_a_null_stay_k(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    big = 1 << 30
    call = lib.abn_hmm_forward_backward_stats
    #       x  T    D  off len n  sh A  B  c0 w  K  rho  mode post ll stays ng stay_k ws  bytes stream
    good = [p, 100, 4, p, p, 2, p, p, p, p, p, 8, 0.5, 0, p, p, None, p, p, p, big, None]

    def with_(**kw):
        a = list(good)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return call(*a)
    for i in (0, 3, 4, 6, 7, 8, 9, 10, 14, 15, 17, 18):                # every pointer but stays
        assert with_(**{'a%d' % i: None}) == _lib.E_ARG, i
        assert b'null pointer' in lib.abn_last_error() and b'abn_hmm_forward_backward_stats' in lib.abn_last_error()
    assert with_(a1=0) == _lib.E_ARG and with_(a1=1 << 31) == _lib.E_ARG
    assert with_(a2=0) == _lib.E_ARG and with_(a5=0) == _lib.E_ARG and with_(a11=0) == _lib.E_ARG
    assert with_(a2=lib.abn_gmm_max_d() + 1) == _lib.E_UNSUPPORTED and with_(a11=lib.abn_hmm_max_k() + 1) == _lib.E_UNSUPPORTED
    for rho in (-0.5, 1.0, float('nan')):
        assert with_(a12=rho) == _lib.E_ARG
        assert b'rho' in lib.abn_last_error()
    assert with_(a13=2) == _lib.E_ARG
    assert with_(a19=None) == _lib.E_WORKSPACE and with_(a20=1024) == _lib.E_WORKSPACE
    assert with_(a19=ctypes.c_void_p(0x10004)) == _lib.E_ARG


# ---- the Python layer --------------------------------------------------------------------------------------------------
def fitted_mixture(K=3, D=2):
    from abnet3_amd.gmm import GmmPosteriorgram
    g = GmmPosteriorgram(K)
    g.weights_ = np.full(K, 1.0 / K)
    g.means_, g.variances_ = np.arange(K * D, dtype=np.float64).reshape(K, D), np.ones((K, D))
    g.shift_, g.gv_ = np.zeros(D, dtype=np.float32), np.ones(D)
    return g


def test_fit_refuses_on_the_host_and_leaves_the_mixture_it_was_given(lib):
    from abnet3_amd import hmm
    g = fitted_mixture()
    before = {k: np.array(getattr(g, k)) for k in ('weights_', 'means_', 'variances_', 'shift_', 'gv_')}
    h = hmm.StickyHmmPosteriorgram(g, 0.75)
    assert h.n_retired_ == 0 and h.n_starved_ == 0
    for bad in ('', 'x', 'mvwsx', 'mm', 'MV', None, 3, ['m']):
        with pytest.raises(ValueError, match='params'):
            h.fit(torch.zeros(5, 2), params=bad)
        with pytest.raises(ValueError, match='params'):
            hmm.check_params('t', bad)
    assert hmm.check_params('t', 'mvws') == set('mvws') and hmm.check_params('t', 'sw') == set('sw')
    with pytest.raises(ValueError, match='D = 4'):
        h.fit(torch.zeros(5, 4))
    with pytest.raises(ValueError, match='float32'):
        h.fit(torch.zeros(5, 2, dtype=torch.float64))
    assert h.gmm is g and h.stay_ == 0.75 and h.log_likelihoods == []
    for k, a in before.items():
        assert np.array_equal(getattr(g, k), a), k
    K, D = 3, 2
    z = lambda *s: torch.zeros(*s)
    for args, match in (((z(6, D).double(), z(6, K), z(D)), 'float32'), ((z(6, D), z(5, K), z(D)), 'post'), ((z(6, D), z(6, K).double(), z(D)), 'post'),
                        ((z(6, D), z(6, 2 * K)[:, ::2], z(D)), 'post'), ((z(6, D), z(6, K), z(D + 1)), 'shift'),
                        ((z(6, D), z(6, hmm.max_k() + 1), z(D)), 'abn_hmm_max_k'), ((z(6, D), z(6, K), z(D), 257), 'n_ranges')):
        with pytest.raises(ValueError, match=match):
            hmm.accumulate(*args)
    with pytest.raises(ValueError, match='abn_gmm_max_d'):
        hmm.accumulate(z(6, 200), z(6, K), z(200))


def test_cli_argument_parsing(lib, tmp_path, capsys):
    from abnet3_amd import hmm
    with pytest.raises(SystemExit):
        hmm.main(['fit'])                                                 # the three files are needed
    with pytest.raises(SystemExit):
        hmm.main(['fit', 'a.npz', 'b.npz', 'c.npz', '--n-iter', 'many'])
    capsys.readouterr()
    # a refused --params stops before any file is read
    with pytest.raises(ValueError, match='params'):
        hmm.main(['fit', str(tmp_path / 'none.npz'), str(tmp_path / 'none2.npz'), str(tmp_path / 'out.npz'), '--params', 'mvq'])
    with pytest.raises(OSError):
        hmm.main(['fit', str(tmp_path / 'none.npz'), str(tmp_path / 'none2.npz'), str(tmp_path / 'out.npz'), '--params', 'mv'])
    assert not (tmp_path / 'out.npz').exists()
