"""KLLoss (abnet3/loss.py:108-137) without a GPU: the float64 restatement (kl_np) against the reference's own
outputs (tests/golden/kl_loss.npz, tools/make_golden.py G12), the class surface, the C ABI's additions and the
class lookup a gridsearch experiment does."""
import copy
import os
import re

import numpy as np
import pytest
import torch.nn as nn

import kl_np
from conftest import load_golden

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def g12():
    return load_golden('kl_loss.npz')


def rel(a, b):
    return float(np.abs(np.asarray(a, np.float64) - b).max() / max(np.abs(b).max(), 1e-300))


def np_eval(g, n):
    f = kl_np.kl_prob if n.startswith('a') else kl_np.kl_logits
    return f(g[n + '.in1'], g[n + '.in2'], g[n + '.y'], float(g[n + '.margin']), bool(g[n + '.avg']))


@pytest.mark.parametrize('n', ['a0', 'a1', 'a2', 'a3', 'a4', 'a5', 'b0', 'b1', 'b2', 'b3', 'u0', 'u1'])
def test_kl_np_matches_the_reference(n):
    """G12 (a) probability rows, (b) logits through nn.Softmax(): loss and gradients at 1e-6.  The near-uniform
    cases (u*, 0.01 randn logits) have gradients that are differences of nearly equal fp32 terms in the reference:
    there its float32 side carries ~4e-6 of its own error, and the float64 side is the one pinned at 1e-12 (the
    fixture holds the float64 run's loss for every logits case, its gradients for the near-uniform ones)."""
    g = g12()
    loss, g1, g2 = np_eval(g, n)
    assert abs(loss - g[n + '.loss']) <= 1e-6 * abs(g[n + '.loss'])
    gtol = 1e-5 if n.startswith('u') else 1e-6
    assert rel(g1, g[n + '.g1']) <= gtol and rel(g2, g[n + '.g2']) <= gtol
    if not n.startswith('a'):
        assert abs(loss - g[n + '.loss.f64']) <= 1e-12 * abs(g[n + '.loss.f64'])
    if n.startswith('u'):
        assert rel(g1, g[n + '.g1.f64']) <= 1e-12 and rel(g2, g[n + '.g2.f64']) <= 1e-12


def test_hinge_rule_on_every_label():
    """labels (1, -1, 0, -1, 2), x = (0.3, 0.3, 0.3, 1.0, 1.0), margin 1: values (0.3, 0.7, 1.0, 0, 1.0), derivatives
    (1, -1, 0, -1, 0) -- a tie at the margin passes -1 (clamp_min's backward), other labels take x + max(0, m - x)."""
    v, d = kl_np.hinge(np.array([1, -1, 0, -1, 2]), np.array([0.3, 0.3, 0.3, 1.0, 1.0]), 1.0)
    assert np.allclose(v, [0.3, 0.7, 1.0, 0.0, 1.0]) and abs(v.sum() - 3.0) < 1e-12
    assert list(d) == [1, -1, 0, -1, 0]


def test_logits_form_is_the_probability_form_through_softmax():
    """The division-free logits gradient equals the probability gradient pushed through the softmax Jacobian."""
    rng = np.random.default_rng(3)
    z1, z2 = rng.standard_normal((9, 13)), rng.standard_normal((9, 13))
    y = rng.choice([1, -1, 0, 2], 9)
    p, q = np.exp(kl_np.log_softmax(z1)), np.exp(kl_np.log_softmax(z2))
    lp, gp, gq = kl_np.kl_prob(p, q, y, 0.7, False)
    lz, gz1, gz2 = kl_np.kl_logits(z1, z2, y, 0.7, False)
    jac = lambda s, g: s * (g - (s * g).sum(1, keepdims=True))
    assert abs(lp - lz) < 1e-12 * abs(lp)
    assert rel(gz1, jac(p, gp)) < 1e-10 and rel(gz2, jac(q, gq)) < 1e-10


def test_kl_loss_class_surface():
    from abnet3_amd.loss import KLLoss, LossBuilder
    loss = KLLoss()
    assert isinstance(loss, LossBuilder) and loss.margin == 1 and loss.avg is True
    loss = KLLoss(margin=3, avg=False)
    assert loss.margin == 3 and loss.avg is False
    who = loss.whoami()
    # the reference's whoami: {'params': self.__dict__, 'class_name': ...} of an nn.Module with margin and avg
    assert sorted(who.keys()) == ['class_name', 'params'] and who['class_name'] == 'KLLoss'
    assert set(who['params']) == set(nn.Module().__dict__) | {'margin', 'avg'}


def test_abi_additions():
    from abnet3_amd import _lib
    text = re.sub(r'/\*.*?\*/', '', open(os.path.join(ROOT, 'include', 'abnet3_hip.h')).read(), flags=re.S)
    assert re.search(r'\bABN_LOSS_KL\s*=\s*2\b', text) and re.search(r'\bABN_ACT_SOFTMAX\s*=\s*4\b', text)
    assert re.search(r'#define ABN_ABI_VERSION 20\b', text)
    assert _lib.LOSS['KLLoss'] == 2 and _lib.ACT_SOFTMAX == 4
    assert 'softmax' not in _lib.ACT and 4 not in _lib.ACT.values()      # the tower descriptors read ACT


def test_gridsearch_builds_kl_loss(tmp_path):
    """A YAML experiment with a softmax model and `loss: {class: KLLoss, arguments: {margin: 1}}`, built the way
    the reference's gridsearch builds it (tests/test_gridsearch_boundary.py: build_experiment)."""
    from test_gridsearch_boundary import build_experiment, load
    d = load()
    params = copy.deepcopy(d['default_params'])
    params['model']['arguments']['last_non_linearity'] = 'softmax'
    params['loss'] = {'class': 'KLLoss', 'arguments': {'margin': 1}}
    _, model, loss, _, _, _ = build_experiment(tmp_path, params, d['reference'], False)
    assert type(loss).__name__ == 'KLLoss' and loss.margin == 1 and loss.avg is True
    assert model.last_non_linearity == 'softmax'
    params['loss'] = {'class': 'KLLoss', 'arguments': {'margin': 0.25, 'avg': False}}
    _, _, loss, _, _, _ = build_experiment(tmp_path / 'b', params, d['reference'], False)
    assert loss.margin == 0.25 and loss.avg is False
