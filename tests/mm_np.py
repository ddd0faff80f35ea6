"""The integration unit of the multimodal network (abnet3/integration.py:71-475) restated in float64 numpy -- the
definition abn_integrate_forward / abn_integrate_backward (csrc/integrate.hip) compute, written independently of
the reference.

  sum     out = w * x1 + (1 - w) * x2                concat  out = [w * x1 | (1 - w) * x2]
  w = 1 (no weight: plain sum / concatenation), a fixed or learnt scalar, or act(z), z [rows, K] (K = 1: one weight
  per row, K = width: one per feature).
  d x1 = g1 * w, d x2 = g2 * (1 - w), d w = g1 * x1 - g2 * x2 (summed over what w is shared by), d z = d w * act'(z)."""
import numpy as np


def act(name, z):
    z = np.asarray(z, np.float64)
    return np.tanh(z) if name == 'tanh' else 1.0 / (1.0 + np.exp(-z))


def act_grad_from_output(name, w):
    return 1.0 - w * w if name == 'tanh' else w * (1.0 - w)


def weights(kind, rows, w=None, z=None, act_name='sigmoid'):
    """(w, 1 - w) as [rows, K] float64 arrays."""
    if kind == 'none':
        one = np.ones((rows, 1))
        return one, one
    if kind in ('fixed', 'scalar'):
        w = np.full((rows, 1), float(np.asarray(w).reshape(-1)[0]))
        return w, 1.0 - w
    w = act(act_name, z)
    return w, 1.0 - w


def forward(mode, x1, x2, w, wc):
    x1, x2 = np.asarray(x1, np.float64), np.asarray(x2, np.float64)
    if mode == 'sum':
        return w * x1 + wc * x2
    return np.concatenate((w * x1, wc * x2), axis=1)


def backward(mode, kind, x1, x2, g, w, wc, act_name='sigmoid'):
    """(dx1, dx2, dz | None, dw | None) for the upstream gradient g."""
    x1, x2, g = (np.asarray(a, np.float64) for a in (x1, x2, g))
    d1 = x1.shape[1]
    g1, g2 = (g, g) if mode == 'sum' else (g[:, :d1], g[:, d1:])
    dx1, dx2 = g1 * w, g2 * wc
    if kind in ('none', 'fixed'):
        return dx1, dx2, None, None
    if w.shape[1] == 1:
        t = (g1 * x1).sum(axis=1, keepdims=True) - (g2 * x2).sum(axis=1, keepdims=True)
    else:
        t = g1 * x1 - g2 * x2
    if kind == 'scalar':
        return dx1, dx2, None, np.array([t.sum()])
    return dx1, dx2, t * act_grad_from_output(act_name, w), None


def unit_case(g, name):
    """The inputs of G13's unit case `name` as (mode, kind, x1, x2, g, w, wc, act)."""
    mode = str(g[name + '.mode'])
    rows = g[name + '.x1'].shape[0]
    if name + '.z' in g:
        kind, act_name = 'attention', str(g[name + '.act'])
        w, wc = weights(kind, rows, z=g[name + '.z'], act_name=act_name)
    elif name + '.w' in g:
        kind, act_name = ('scalar' if 'scalar' in name else 'fixed'), 'sigmoid'
        w, wc = weights(kind, rows, w=g[name + '.w'])
    else:
        kind, act_name = 'none', 'sigmoid'
        w, wc = weights(kind, rows)
    return mode, kind, g[name + '.x1'], g[name + '.x2'], g[name + '.g'], w, wc, act_name
