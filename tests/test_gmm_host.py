"""GmmPosteriorgram without a GPU: the float64 restatement's invariants (tests/gmm_np.py), the documented
initialisation, the variance floor and the starved-component rule, the save / load round trip, the ValueErrors, and
the library's argument checks and workspace sizing (no kernel is launched here)."""
import ctypes

import numpy as np
import pytest
import torch

import gmm_np


@pytest.fixture(scope='module')
def lib():
    from abnet3_amd import build, _lib
    build.build()
    return _lib.load()


def mixture(T=600, K=4, D=3, seed=0, spread=8.0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(size=(K, D)) * spread
    lab = rng.integers(0, K, size=T)
    return (centres[lab] + rng.normal(size=(T, D))).astype(np.float32), lab


def test_float64_invariants():
    x, _ = mixture()
    x[7, 1] = np.nan
    x[100, 0] = np.inf
    shift, gv = gmm_np.moments(x)
    xc, bad = gmm_np.centre(x, shift)
    assert list(np.flatnonzero(bad)) == [7, 100]
    w, m, v = gmm_np.initial(xc, bad, gv, 4)
    A, B, c = gmm_np.tables(w, m, v)
    lse, g = gmm_np.lse_post(gmm_np.scores(xc, bad, A, B, c), bad)
    assert np.isnan(lse[bad]).all() and np.isfinite(lse[~bad]).all()
    assert np.abs(g[~bad].sum(axis=1) - 1.0).max() < 1e-12 and not g[bad].any()
    N, S1, S2 = gmm_np.statistics(g, xc, bad)
    assert abs(N.sum() - (len(x) - 2)) < 1e-9
    assert np.isfinite(S1).all() and np.isfinite(S2).all()


@pytest.mark.parametrize('seed', [0, 1, 2])
def test_log_likelihood_does_not_decrease_in_float64(seed):
    x, _ = mixture(seed=seed)
    ll = gmm_np.fit(x, 4, n_iter=12, tol=-np.inf, seed=seed)['log_likelihoods']
    assert len(ll) == 12
    for a, b in zip(ll, ll[1:]):
        assert b >= a - 1e-9 * abs(a), ll


def test_initialisation_is_the_documented_draw():
    x, _ = mixture(T=50)
    x[3] = np.nan
    shift, gv = gmm_np.moments(x)
    xc, bad = gmm_np.centre(x, shift)
    w, m, v = gmm_np.initial(xc, bad, gv, 5, seed=3)
    good = np.flatnonzero(~bad)
    pick = np.sort(np.random.default_rng(3).choice(49, 5, replace=False))
    assert np.array_equal(m, xc[good[pick]].astype(np.float64))
    assert len(set(good[pick])) == 5 and 3 not in good[pick]
    assert np.array_equal(v, np.tile(gv, (5, 1))) and np.array_equal(w, np.full(5, 0.2))
    with pytest.raises(ValueError):
        gmm_np.initial(xc, bad, gv, 50)


def test_variance_floor_and_starved_components():
    gv = np.array([4.0, 1.0])
    m_prev = np.array([[9.0, 9.0], [1.0, 1.0], [2.0, 2.0]])
    v_prev = np.full((3, 2), 7.0)
    N = np.array([10.0, 0.5, 30.0])
    S1 = np.array([[10.0, 20.0], [0.1, 0.1], [30.0, 0.0]])
    S2 = np.array([[10.0 + 1e-6, 100.0], [1.0, 1.0], [60.0, 30.0]])
    w, m, v, starved = gmm_np.mstep(N, S1, S2, 40.5, gv, m_prev, v_prev, var_floor=0.01, min_count=1.0)
    assert starved == 1
    assert np.array_equal(m[1], m_prev[1]) and np.array_equal(v[1], v_prev[1])        # kept
    assert np.allclose(m[0], [1.0, 2.0]) and v[0, 0] == 0.04 and np.isclose(v[0, 1], 6.0)   # floored at 0.01 gv
    assert np.allclose(v[2], [1.0, 1.0])
    assert np.isclose(w.sum(), 1.0) and np.allclose(w, N / 40.5 / (N / 40.5).sum())


def test_save_load_round_trip(lib, tmp_path):
    from abnet3_amd.gmm import GmmPosteriorgram
    g = GmmPosteriorgram(3, n_iter=7, tol=1e-3, var_floor=0.02, min_count=2.0, seed=5)
    rng = np.random.default_rng(0)
    g.weights_ = np.array([0.2, 0.3, 0.5])
    g.means_ = rng.normal(size=(3, 4))
    g.variances_ = rng.uniform(0.5, 2.0, size=(3, 4))
    g.shift_ = rng.normal(size=4).astype(np.float32)
    g.gv_ = rng.uniform(0.5, 2.0, size=4)
    g.log_likelihoods = [-3.0, -2.5]
    path = str(tmp_path / 'gmm.npz')
    g.save(path)
    h = GmmPosteriorgram.load(path)
    assert h.whoami() == g.whoami() and h.whoami()['class_name'] == 'GmmPosteriorgram'
    for k in ('weights_', 'means_', 'variances_', 'shift_', 'gv_'):
        assert np.array_equal(getattr(g, k), getattr(h, k)) and getattr(g, k).dtype == getattr(h, k).dtype, k
    assert h.log_likelihoods == g.log_likelihoods
    with pytest.raises(ValueError):
        GmmPosteriorgram(3).save(path)


def test_value_errors(lib):
    from abnet3_amd import gmm
    D, K = gmm.max_d(), gmm.max_k()
    assert D >= 100 and K >= 4096
    with pytest.raises(ValueError, match='T < K'):
        gmm.GmmPosteriorgram(8).fit(torch.zeros(3, 4))
    with pytest.raises(ValueError, match='abn_gmm_max_d'):
        gmm.GmmPosteriorgram(2).fit(torch.zeros(10, D + 1))
    with pytest.raises(ValueError, match='abn_gmm_max_k'):
        gmm.GmmPosteriorgram(K + 1).fit(torch.zeros(2 * K, 4))
    with pytest.raises(ValueError, match='float32'):
        gmm.GmmPosteriorgram(2).fit(torch.zeros(10, 4, dtype=torch.float64))
    with pytest.raises(ValueError, match='float32'):
        gmm.GmmPosteriorgram(2).fit({'a': np.zeros((10, 4))})
    with pytest.raises(ValueError):
        gmm.GmmPosteriorgram(0)
    with pytest.raises(ValueError, match='fit or load'):
        gmm.GmmPosteriorgram(2).transform(torch.zeros(10, 4))


def test_library_refuses_bad_arguments_before_any_launch(lib):
    from abnet3_amd import _lib
    p = ctypes.c_void_p(0x10000)
    D, K = lib.abn_gmm_max_d(), lib.abn_gmm_max_k()
    assert lib.abn_gmm_posteriors(None, 10, 4, p, p, p, p, 2, p, None, None) == _lib.E_ARG
    assert b'null' in lib.abn_last_error()
    assert lib.abn_gmm_posteriors(p, 0, 4, p, p, p, p, 2, p, None, None) == _lib.E_ARG
    assert b'T = 0' in lib.abn_last_error()
    assert lib.abn_gmm_posteriors(p, 10, D + 1, p, p, p, p, 2, p, None, None) == _lib.E_UNSUPPORTED
    assert b'abn_gmm_max_d' in lib.abn_last_error()
    assert lib.abn_gmm_posteriors(p, 10, 4, p, p, p, p, K + 1, p, None, None) == _lib.E_UNSUPPORTED
    assert lib.abn_gmm_accumulate(p, 10, 4, p, p, p, p, 2, None, 0, p, 1 << 20, None) == _lib.E_ARG
    assert lib.abn_gmm_accumulate(p, 10, 4, p, p, p, p, 2, p, 0, p, 8, None) == _lib.E_WORKSPACE
    assert b'abn_gmm_ws_bytes' in lib.abn_last_error()
    assert lib.abn_gmm_accumulate(p, 10, 4, p, p, p, p, 2, p, 257, p, 1 << 20, None) == _lib.E_ARG
    assert lib.abn_gmm_mstep(p, 1 << 20, p, 10, 2, 4, 0, p, -1.0, 1.0, p, p, p, p, p, p, p, p, None) == _lib.E_ARG
    assert b'var_floor' in lib.abn_last_error()
    assert lib.abn_gmm_mstep(p, 1 << 20, p, 10, 2, 4, 0, None, 0.01, 1.0, p, p, p, p, p, p, p, p, None) == _lib.E_ARG
    assert lib.abn_gmm_mstep(None, 0, p, 10, 2, 4, 0, p, 0.01, 1.0, p, p, p, p, p, p, p, p, None) == _lib.E_WORKSPACE
    assert lib.abn_gmm_ws_bytes(0, 2, 4, 0) == -1 and lib.abn_gmm_ws_bytes(10, 2, D + 1, 0) == -1
    assert lib.abn_gmm_ws_bytes(10, K + 1, 4, 0) == -1


def test_workspace_is_monotone_in_t_and_k(lib):
    for D in (1, 39, 100):
        prev = 0
        for T in (1, 127, 128, 129, 1000, 100000, 1140000):
            ws = lib.abn_gmm_ws_bytes(T, 256, D, 0)
            assert ws >= prev > -1, (T, D)
            prev = ws
        prev = 0
        for K in (1, 128, 129, 1024, 4096):
            ws = lib.abn_gmm_ws_bytes(1140000, K, D, 0)
            assert ws >= prev > -1, (K, D)
            prev = ws
    # one slab [128][2 D + 1] of fp32 per (component tile, range): explicit ranges are taken as given
    assert lib.abn_gmm_ws_bytes(300, 130, 39, 3) == 2 * 3 * 128 * 79 * 4
    assert lib.abn_gmm_ws_bytes(300, 130, 39, 2) == 2 * 2 * 128 * 79 * 4
