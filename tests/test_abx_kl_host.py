"""The symmetrised Kullback-Leibler frame distance of the ABX evaluation without a GPU: the properties of the numpy
restatement (tests/abx_kl_np.py) the definition was chosen for, its agreement with a float64 evaluation to a derived
bound, the two new entry points in header and binding, and the argument check of ABXEvaluator."""
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import abx_kl_np  # noqa: E402
from conftest import ROOT  # noqa: E402


def softmax_rows(rng, n, D, scale):
    z = scale * rng.standard_normal((n, D))
    e = np.exp(z - z.max(axis=1, keepdims=True))
    return (e / e.sum(axis=1, keepdims=True)).astype(np.float32)


def frame_sets(rng, D):
    """Random softmax rows (soft and peaked), rows with exact zeros, one-hot rows."""
    soft = softmax_rows(rng, 12, D, 1.0)
    peaked = softmax_rows(rng, 12, D, 30.0)             # most entries far below the floor
    zeros = softmax_rows(rng, 8, D, 2.0)
    zeros[:, ::2] = 0.0
    onehot = np.zeros((min(D, 6), D), dtype=np.float32)
    onehot[np.arange(len(onehot)), np.arange(len(onehot))] = 1.0
    return np.concatenate([soft, peaked, zeros, onehot, soft[:3]])      # (the last three repeat the first three)


@pytest.mark.parametrize('D', [1, 3, 40, 100, 257])
def test_restatement_properties(D):
    rng = np.random.default_rng(D)
    x = frame_sets(rng, D)
    P, L, bad = abx_kl_np.tables(x)
    assert not bad.any() and P.dtype == np.float32 and L.dtype == np.float32
    assert (P >= np.float32(1e-6)).all() and np.array_equal(P[x > 1e-6], x[x > 1e-6])
    d = abx_kl_np.frame_distances(P, L, P, L)
    assert d.dtype == np.float32
    assert (d >= 0).all()                                            # every term is >= 0
    assert (np.diag(d) == 0).all()                                   # identical frames: exactly 0 ...
    assert (d[:3, -3:].diagonal() == 0).all()                        # ... also as two rows of the table
    assert np.array_equal(d.view(np.int32), d.T.copy().view(np.int32))      # d(p, q) == d(q, p) bit for bit

    # Agreement with 0.5 (KL(p||q) + KL(q||p)) = 0.5 sum_k (p - q)(log p - log q) of the floored rows in float64.
    # With u = 2^-24 (float32's unit roundoff), per term t = (p - q)(lp - lq), lp = log p:
    #   * the table holds L_p = lp (1 + e), |e| <= u, so L_p - L_q = (lp - lq) + err, |err| <= u (|lp| + |lq|);
    #   * the two subtractions and the product are rounded once each: a factor (1 + e1)(1 + e2)(1 + e3);
    #   * the term then passes through at most D additions of the running sum, each a factor (1 + e'); all terms are
    #     >= 0, so nothing cancels and the factors apply to the terms themselves.
    # Hence |computed term - t| <= gamma(D + 3) |t| + u (1 + gamma(D + 3)) |p - q| (|lp| + |lq|) with
    # gamma(n) = n u / (1 - n u) (Higham); the 0.5 is exact.  A result in the subnormal range may lose up to 2^-149
    # per operation, and the float64 evaluation itself has D 2^-53 relative error on the same two sums.
    u = 2.0 ** -24
    gamma = (D + 3) * u / (1 - (D + 3) * u)
    P64 = P.astype(np.float64)
    l64 = np.log(P64)
    dp = P64[:, None, :] - P64[None, :, :]
    A = (np.abs(dp) * np.abs(l64[:, None, :] - l64[None, :, :])).sum(axis=2)
    B = (np.abs(dp) * (np.abs(l64[:, None, :]) + np.abs(l64[None, :, :]))).sum(axis=2)
    ref = 0.5 * (dp * (l64[:, None, :] - l64[None, :, :])).sum(axis=2)
    bound = 0.5 * (gamma * A + u * (1 + gamma) * B) + 4 * D * 2.0 ** -149 + D * 2.0 ** -53 * (A + B)
    err = np.abs(d.astype(np.float64) - ref)
    assert (err <= bound).all(), (err - bound).max()
    assert (bound[ref > 0] / ref[ref > 0]).max() < 1e-3               # (the bound says something)


def test_tables_flag_bad_rows_and_floor_zeros():
    x = np.full((6, 4), 0.25, dtype=np.float32)
    x[0, 1] = np.nan
    x[1, 2] = np.inf
    x[2, 0] = -1e-3
    x[3, 3] = 0.0
    x[4, 0] = 5e-7
    P, L, bad = abx_kl_np.tables(x, floor=1e-6)
    assert bad.tolist() == [True, True, True, False, False, False]
    assert P[3, 3] == np.float32(1e-6) and P[4, 0] == np.float32(1e-6)
    assert L[3, 3] == np.float32(np.log(np.float64(np.float32(1e-6))))


def test_restatement_dtw_tie_break_and_length():
    # all costs equal: the diagonal is taken first; then up (token 1 longer) or left (token 2 longer)
    assert abx_kl_np.dtw(np.zeros((4, 4), np.float32)) == (0.0, 4)
    assert abx_kl_np.dtw(np.zeros((6, 4), np.float32)) == (0.0, 6)
    assert abx_kl_np.dtw(np.zeros((3, 7), np.float32)) == (0.0, 7)
    assert abx_kl_np.dtw(np.zeros((0, 7), np.float32)) == (0.0, 0)
    d = np.array([[1, 9, 9], [9, 1, 9], [0, 0, 1]], dtype=np.float32)
    assert abx_kl_np.dtw(d) == (3.0, 3)


def test_header_and_binding_carry_the_new_symbols():
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    for name in ('abn_kl_tables', 'abn_dtw_cost_kl_batched'):
        assert re.search(r'\b%s\s*\(' % name, text), name
        assert name in _lib.SYMBOLS, name
    assert re.search(r'#define ABN_ABI_VERSION 20\b', text)
    assert _lib.ABI_VERSION == 20


def test_unknown_distance_raises_without_a_device():
    from abnet3_amd.abx import ABXEvaluator, ABXResult, Items, dtw_cost_batch
    items = Items(['f'], [0.0], [0.1], ['a'], ['-'], ['-'], ['s'])
    with pytest.raises(ValueError, match='distance'):
        ABXEvaluator(items, {'f': np.zeros((20, 4), np.float32)}, {'f': np.arange(20) * 0.01}, distance='nonsense')
    with pytest.raises(ValueError, match='distance'):
        dtw_cost_batch(None, [], [], None, [], [], distance='nonsense')
    assert ABXResult('within', 0.0, [], {}, 0, 0, 0, []).distance == 'cosine'


def test_command_line_takes_the_distance(capsys):
    from abnet3_amd import abx
    with pytest.raises(SystemExit):
        abx.main(['feats.h5f', 'items', '--distance', 'euclidean'])
    assert 'kl' in capsys.readouterr().err
