"""The in-batch contrastive pair loss (InfoNCE / NT-Xent) restated three times, the error bars of abnt_nce_loss derived from
the kernel's operation order, and the inputs the tests share.  abnet3_amd/loss.py (InfoNCELoss) states the definition.

    loops(...)         float64, one Python loop per index: explicit and slow, for small cases
    reference(...)     float64 numpy, the same formulas row-wise: loss, terms, the closed-form gradient and the row scales
    torch_loss(...)    torch ops (normalise, mm, two logsumexp), any device and dtype; its gradient comes from autograd
    closed_form_f32()  the closed-form gradient in float32 torch ops on the CPU, with the three mutants of the host test

The bars (u = 2^-24, B rows, D columns).  The kernel subtracts the mean mu of all 2 B unit rows from every row (in float64,
rounded once) and forms z = (<alpha_i, beta_j> + (<alpha_i, mu> + <mu, beta_j>)) / tau: the similarity less |mu|^2, a shift
that every logit shares and that changes neither a term nor a gradient.  |mu| <= 1, so |alpha|, |beta| <= 2 in the worst
case (and sum_k |alpha_k beta_k| <= 4), far less where the rows are nearly parallel -- which is where fp32 needs it.
  z     the rounded rows carry u per element (2 u sum |alpha_k beta_k| <= 8 u), the D-term fp32 chain D u sum |alpha_k
        beta_k| <= 4 D u, the two row terms 2 u each, their sum 4 u, the sum with the tile entry 5 u, the division 5 u:
                                                                eps_z = (4 D + 26) u / tau
  S     a term exp(z_j - m) is first taken against its tile's maximum m0 and later rescaled by exp(m_k - m_{k+1}) every
        time the running maximum rises (tiles, the two halves of a row, the ranges).  The maxima only rise, so the
        subtractions' roundings add up to u (m_final - z_j) <= 2 u / tau in the exponent, however many rescales there
        are; each of the R + 1 <= ceil(B / 128) + 18 exps and products adds 3 u, the additions at most (B + 16) u:
                                                                eps_S = (2 / tau + 3 (R + 1) + B + 16) u
  lse   log sum exp is 1-Lipschitz in the sup norm of z; log adds 2 u |log S| <= 2 u log B, the last addition u |lse| with
        |lse| <= 2 / tau + log B (the shifted similarity lies in -2 .. 1):
                                                                eps_lse = eps_z + eps_S + (3 log B + 2 / tau) u
  term  l = ((la - z_ii) + (lb - z_ii)) / 2, brackets at most 2 / tau + log B:
                                                                eps_term = eps_lse + eps_z + 3 u (2 / tau + log B)
  loss  the float64 sum of n terms, rounded once:               n eps_term (eps_term when avg) + u |loss|
  G     p = exp(z - la) has relative error eps_z + eps_lse from its exponent, u (2 / tau + log B) from the subtraction and
        2 u from exp:  eps_pq.  Row i of G sums to at most c (r_i + sum_j r_j q_ij) =: scale_i in p and q together (sum_j
        p_ij = 1) and 3 scale_i with the diagonal's -2 r_i, whose cancellation against p_ii + q_ii costs 2 u more.
  g     g_i = (sum_j G_ij) mu + sum_j G_ij beta_j: (eps_pq + 4 u) scale_i from G; the second sum is a B-term fp32 chain
        over rows of length <= 2, 6 (B + 18) u scale_i per component with the slabs' sums and beta's own error; the first
        sum and everything behind it (the slabs' sum, <a^, g>, the projection, inv, 1 / n) is float64, rounded once.
  de    (g - a^ <a^, g>) inv: the G part of <a^, g>'s error is again bounded by (eps_pq + 4 u) scale_i (|<a^, b^_j>| <= 1),
        the chain part by sqrt(D) times a component's:
            grad_bar_i = scale_i inv_i (2 (eps_pq + 4 u) + (1 + sqrt(D)) 6 (B + 18) u + 12 u)
                         + inv_i c (2 B + 2) (1 + sqrt(D)) 2^-126
        The last term is fp32's underflow: an exp below the smallest normal number 2^-126 is flushed or rounded to a
        subnormal, off by at most 2^-126 absolutely, in each of a row's 2 B entries of p and q (it matters only where a
        row's whole scale is of that size: two far-apart rows at tau = 0.01).
ABSOLUTE per row, in units of scale_i inv_i -- not relative to the row's own entries, which can be 1e-13 of that scale when
the positive already dominates.  Worst-case sums throughout: the kernel and the float32 restatements use a small share."""
import math

import numpy as np

EPS = 1e-6
U = 2.0 ** -24


# ---- inputs ------------------------------------------------------------------------------------------------------------------
def make_case(B, D, seed=0, noise=0.3):
    """Both sides drawn around min(8, B) random prototype rows with noise 0.3: the loss is informative (plain Gaussian rows
    at D = 100 are all but orthogonal and give losses near 0)."""
    rng = np.random.default_rng(1000 * B + D + seed)
    P = min(8, B)
    proto = rng.standard_normal((P, D))
    which = rng.integers(0, P, size=B)
    e1 = (proto[which] + noise * rng.standard_normal((B, D))).astype(np.float32)
    e2 = (proto[which] + noise * rng.standard_normal((B, D))).astype(np.float32)
    return e1, e2


def labels(B, kind):
    y = -np.ones(B, dtype=np.int64)
    if kind == 'all':
        y[:] = 1
    elif kind == 'alt':
        y[::2] = 1
    elif kind == 'one':
        y[B // 2] = 1
    else:
        assert kind == 'none'
    return y


MAX_D = 256                          # abnt_nce_max_d(); tests/test_nce_host.py checks it against the library
# (B, D, tau, labels): every B edge with two widths, every temperature, every label pattern
CASES = ((1, 1, 0.5, 'all'), (1, 100, 0.07, 'all'), (2, 2, 0.5, 'all'), (2, 33, 0.01, 'alt'),
         (127, 3, 0.07, 'all'), (127, 100, 0.5, 'alt'), (128, 33, 0.07, 'one'), (128, MAX_D, 0.01, 'all'),
         (129, 1, 0.5, 'all'), (129, 100, 0.01, 'alt'), (257, 2, 0.07, 'alt'), (257, 100, 0.07, 'all'),
         (257, MAX_D, 0.5, 'none'))
BIG = (1025, 100, 0.07, 'all')       # the split case


# ---- 1: the loops ---------------------------------------------------------------------------------------------------------------
def loops(e1, e2, y, tau, groups=None, avg=True):
    """(loss, terms [B]) in float64, one loop per index."""
    e1, e2 = np.asarray(e1, dtype=np.float64), np.asarray(e2, dtype=np.float64)
    B, D = e1.shape
    a, b = np.zeros((B, D)), np.zeros((B, D))
    for i in range(B):
        na = math.sqrt(sum(e1[i, k] * e1[i, k] for k in range(D)))
        nb = math.sqrt(sum(e2[i, k] * e2[i, k] for k in range(D)))
        for k in range(D):
            a[i, k] = e1[i, k] / max(na, EPS)
            b[i, k] = e2[i, k] / max(nb, EPS)
    z = [[sum(a[i, k] * b[j, k] for k in range(D)) / tau for j in range(B)] for i in range(B)]
    keep = [[j == i or groups is None or groups[i] != groups[j] for j in range(B)] for i in range(B)]
    terms = np.zeros(B)
    for i in range(B):
        ma = max(z[i][j] for j in range(B) if keep[i][j])
        la = ma + math.log(sum(math.exp(z[i][j] - ma) for j in range(B) if keep[i][j]))
        mb = max(z[j][i] for j in range(B) if keep[j][i])
        lb = mb + math.log(sum(math.exp(z[j][i] - mb) for j in range(B) if keep[j][i]))
        terms[i] = 0.5 * (la + lb) - z[i][i]
    n = sum(1 for i in range(B) if y[i] == 1)
    loss = sum(terms[i] for i in range(B) if y[i] == 1)
    if n == 0:
        return 0.0, terms
    return (loss / n if avg else loss), terms


# ---- 2: float64 numpy with the closed-form gradient ----------------------------------------------------------------------------
def _lse(z, keep, axis):
    zz = np.where(keep, z, -np.inf)
    m = zz.max(axis=axis, keepdims=True)
    return (m + np.log(np.exp(zz - m).sum(axis=axis, keepdims=True))).squeeze(axis)


def reference(e1, e2, y, tau, groups=None, avg=True, dtype=np.float64):
    """dict(loss, terms, de1, de2, n, scale_a, scale_b, inv_a, inv_b): the definition and the closed-form gradient."""
    e1, e2 = np.asarray(e1, dtype=dtype), np.asarray(e2, dtype=dtype)
    B, D = e1.shape
    na, nb = np.sqrt((e1 * e1).sum(axis=1)), np.sqrt((e2 * e2).sum(axis=1))
    inv_a, inv_b = 1.0 / np.maximum(na, EPS), 1.0 / np.maximum(nb, EPS)
    a, b = e1 * inv_a[:, None], e2 * inv_b[:, None]
    z = (a @ b.T) / tau
    eye = np.eye(B, dtype=bool)
    keep = np.ones((B, B), dtype=bool) if groups is None else (eye | (np.asarray(groups)[:, None] != np.asarray(groups)[None, :]))
    la, lb = _lse(z, keep, 1), _lse(z, keep, 0)
    terms = 0.5 * (la + lb) - np.diag(z)
    r = (np.asarray(y) == 1).astype(dtype)
    n = int(r.sum())
    mean = avg and n > 0
    loss = float((r * terms).sum() / n) if mean else float((r * terms).sum())
    c = (0.5 / tau) * (1.0 / n if mean else 1.0)
    if n == 0:
        loss, c = 0.0, 0.0
    p = np.where(keep, np.exp(np.where(keep, z - la[:, None], 0.0)), 0.0)
    q = np.where(keep, np.exp(np.where(keep, z - lb[None, :], 0.0)), 0.0)
    G = c * (r[:, None] * p + r[None, :] * q - 2.0 * np.diag(r))
    ga, gb = G @ b, G.T @ a

    def back(g, unit, inv, norm):
        proj = g - unit * (unit * g).sum(axis=1, keepdims=True)
        return np.where((norm >= EPS)[:, None], proj, g) * inv[:, None]
    return dict(loss=loss, terms=terms, de1=back(ga, a, inv_a, na), de2=back(gb, b, inv_b, nb), n=n,
                scale_a=c * (r + (r[None, :] * q).sum(axis=1)), scale_b=c * (r + (r[:, None] * p).sum(axis=0)),
                inv_a=inv_a, inv_b=inv_b, c=c)


# ---- 3: torch ops ------------------------------------------------------------------------------------------------------------------
def torch_loss(e1, e2, y, tau, groups=None, avg=True):
    """The plain torch expression on e1's device and dtype; differentiable.  Materialises the B x B logits."""
    import torch
    B = e1.shape[0]
    a = e1 / e1.norm(dim=1, keepdim=True).clamp_min(EPS)
    b = e2 / e2.norm(dim=1, keepdim=True).clamp_min(EPS)
    z = (a @ b.t()) / tau
    zm = z
    if groups is not None:
        g = groups.to(e1.device)
        drop = (g[:, None] == g[None, :]) & ~torch.eye(B, dtype=torch.bool, device=e1.device)
        zm = z.masked_fill(drop, float('-inf'))
    terms = 0.5 * (torch.logsumexp(zm, dim=1) + torch.logsumexp(zm, dim=0)) - z.diagonal()
    r = (y.to(e1.device) == 1).to(e1.dtype)
    n = r.sum()
    loss = (r * terms).sum()
    if float(n) == 0.0:
        return loss * 0.0
    return loss / n if avg else loss


def torch_value_and_grad(e1, e2, y, tau, groups=None, avg=True, dtype=None):
    """(loss, de1, de2) as numpy arrays from torch_loss and autograd on the CPU."""
    import torch
    dtype = dtype or torch.float64
    t1 = torch.tensor(np.asarray(e1), dtype=dtype, requires_grad=True)
    t2 = torch.tensor(np.asarray(e2), dtype=dtype, requires_grad=True)
    g = None if groups is None else torch.tensor(np.asarray(groups))
    loss = torch_loss(t1, t2, torch.tensor(np.asarray(y)), tau, g, avg)
    loss.backward()
    return float(loss.detach()), t1.grad.numpy(), t2.grad.numpy()


MUTANTS = ('drop_column', 'la_for_lb', 'diagonal_on_non_anchors')


def closed_form_f32(e1, e2, y, tau, groups=None, avg=True, mutant=None):
    """(loss, de1, de2): the closed form in float32 torch ops on the CPU.  mutant: one of MUTANTS, a wrong kernel."""
    import torch
    assert mutant is None or mutant in MUTANTS
    f = torch.float32
    e1, e2 = torch.tensor(np.asarray(e1), dtype=f), torch.tensor(np.asarray(e2), dtype=f)
    B = e1.shape[0]
    na, nb = e1.norm(dim=1), e2.norm(dim=1)
    inv_a, inv_b = 1.0 / na.clamp_min(EPS), 1.0 / nb.clamp_min(EPS)
    a, b = e1 * inv_a[:, None], e2 * inv_b[:, None]
    z = (a @ b.t()) / tau
    eye = torch.eye(B, dtype=torch.bool)
    keep = torch.ones(B, B, dtype=torch.bool)
    if groups is not None:
        g = torch.tensor(np.asarray(groups))
        keep = eye | (g[:, None] != g[None, :])
    zm = z.masked_fill(~keep, float('-inf'))
    za = zm.clone()
    if mutant == 'drop_column' and B > 1:
        za[0, B - 1] = float('-inf')                       # one column missing from la[0]'s sum
    la, lb = torch.logsumexp(za, dim=1), torch.logsumexp(zm, dim=0)
    terms = 0.5 * (la + lb) - z.diagonal()
    r = torch.tensor((np.asarray(y) == 1).astype(np.float32))
    n = float(r.sum())
    if n == 0:
        return 0.0, np.zeros(e1.shape, np.float32), np.zeros(e1.shape, np.float32)
    c = (0.5 / tau) * (1.0 / n if avg else 1.0)
    loss = float((r * terms).sum() * ((1.0 / n) if avg else 1.0))
    p = torch.exp(zm - la[:, None])
    q = torch.exp(zm - (la if mutant == 'la_for_lb' else lb)[None, :])
    diag = torch.ones(B) if mutant == 'diagonal_on_non_anchors' else r
    G = c * (r[:, None] * p + r[None, :] * q - 2.0 * torch.diag(diag))
    ga, gb = G @ b, G.t() @ a

    def back(g, unit, inv, norm):
        proj = g - unit * (unit * g).sum(dim=1, keepdim=True)
        return (torch.where((norm >= EPS)[:, None], proj, g) * inv[:, None]).numpy()
    return loss, back(ga, a, inv_a, na), back(gb, b, inv_b, nb)


# ---- the bars --------------------------------------------------------------------------------------------------------------------
def _eps(B, D, tau):
    logb = math.log(max(B, 2))
    R = -(-B // 128) + 17
    eps_z = (4 * D + 26) * U / tau
    eps_s = (2.0 / tau + 3 * (R + 1) + B + 16) * U
    eps_lse = eps_z + eps_s + (3 * logb + 2.0 / tau) * U
    eps_term = eps_lse + eps_z + 3 * U * (2.0 / tau + logb)
    eps_pq = eps_z + eps_lse + U * (2.0 / tau + logb + 2)
    return eps_term, eps_pq


def term_bar(B, D, tau, terms):
    """[B]: the bar of every l[i]."""
    return _eps(B, D, tau)[0] + U * np.abs(terms)


def loss_bar(B, D, tau, n, avg, loss):
    return _eps(B, D, tau)[0] * (1 if avg else max(n, 1)) + U * abs(loss)


def grad_bar(B, D, tau, scale, inv, c):
    """[B, 1]: the absolute bar of row i of a gradient, scale = reference()'s scale_a / scale_b, inv its inv_a / inv_b, c its c."""
    eps_pq = _eps(B, D, tau)[1]
    rel = 2 * (eps_pq + 4 * U) + (1 + math.sqrt(D)) * 6 * (B + 18) * U + 12 * U
    floor = c * (2 * B + 2) * (1 + math.sqrt(D)) * 2.0 ** -126
    return (np.asarray(inv) * (np.asarray(scale) * rel + floor))[:, None]


def check(got_loss, got_de1, got_de2, ref, B, D, tau, avg, what=''):
    """Asserts kernel (or restatement) outputs against reference()'s dict within the bars; returns the largest shares used."""
    lb = loss_bar(B, D, tau, ref['n'], avg, ref['loss'])
    used = [abs(float(got_loss) - ref['loss']) / lb if lb > 0 else 0.0]
    assert abs(float(got_loss) - ref['loss']) <= lb, '%s loss %r against %r, bar %.3g' % (what, float(got_loss), ref['loss'], lb)
    for got, key, sc, inv in ((got_de1, 'de1', 'scale_a', 'inv_a'), (got_de2, 'de2', 'scale_b', 'inv_b')):
        if got is None:
            continue
        bar = grad_bar(B, D, tau, ref[sc], ref[inv], ref['c'])
        err = np.abs(np.asarray(got, dtype=np.float64) - ref[key])
        assert np.isfinite(np.asarray(got)).all(), '%s %s is not finite' % (what, key)
        bad = err > bar
        assert not bad.any(), '%s %s: %d entries outside the bar, the worst %.3g x' % (
            what, key, int(bad.sum()), float((err / np.maximum(bar, 1e-300)).max()))
        used.append(float((err / np.maximum(bar, 1e-300)).max()) if bar.max() > 0 else 0.0)
    return used
