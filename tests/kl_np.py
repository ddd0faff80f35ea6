"""KLLoss (abnet3/loss.py:108-137) restated in float64 numpy, both input forms -- the definition the HIP kernel
(csrc/loss.hip, kl_pair_loss_kernel) computes, written independently of the reference.

loss = H(KL(p||q)) + H(KL(q||p)) with H = nn.HingeEmbeddingLoss(margin): label 1 -> x, label -1 ->
max(0, margin - x), any other label -> x + max(0, margin - x); a mean over the B pairs with avg, else a sum.
The hinge's derivative at x == margin is the one of clamp_min's backward (the gradient passes where margin - x >= 0)."""
import numpy as np


def hinge(y, x, margin):
    """(H(x), H'(x)) per row."""
    y = np.asarray(y, dtype=np.float64)
    inside = (margin - x) >= 0.0
    clamp = np.where(inside, margin - x, 0.0)
    val = np.where(y != 1, clamp, 0.0) + np.where(y != -1, x, 0.0)
    der = np.where(y != 1, np.where(inside, -1.0, 0.0), 0.0) + np.where(y != -1, 1.0, 0.0)
    return val, der


def _finish(kpq, kqp, y, margin, avg):
    B = kpq.shape[0]
    h1, d1 = hinge(y, kpq, margin)
    h2, d2 = hinge(y, kqp, margin)
    scale = 1.0 / B if avg else 1.0
    return (h1.sum() + h2.sum()) * scale, d1[:, None] * scale, d2[:, None] * scale


def kl_prob(p, q, y, margin=1.0, avg=True):
    """Probability rows p, q [B, D] -> (loss, d loss / d p, d loss / d q)."""
    p, q = np.asarray(p, np.float64), np.asarray(q, np.float64)
    lr = np.log(p / q)
    kpq, kqp = (p * lr).sum(1), (-q * lr).sum(1)
    loss, s1, s2 = _finish(kpq, kqp, y, margin, avg)
    return loss, s1 * (lr + 1.0) - s2 * q / p, s2 * (1.0 - lr) - s1 * p / q


def log_softmax(z):
    z = np.asarray(z, np.float64)
    m = z.max(1, keepdims=True)
    return z - (m + np.log(np.exp(z - m).sum(1, keepdims=True)))


def kl_logits(z1, z2, y, margin=1.0, avg=True):
    """Logits z1, z2 [B, D] of p = softmax(z1), q = softmax(z2) -> (loss, d loss / d z1, d loss / d z2), in the
    division-free form:  dz1 = s1 (p d - p KL_pq) - s2 (q - p),  dz2 = s2 (-q d - q KL_qp) - s1 (p - q),
    d = log p - log q, s = scale * H'(KL)."""
    lp, lq = log_softmax(z1), log_softmax(z2)
    p, q, d = np.exp(lp), np.exp(lq), lp - lq
    kpq, kqp = (p * d).sum(1), (-q * d).sum(1)
    loss, s1, s2 = _finish(kpq, kqp, y, margin, avg)
    return (loss, s1 * (p * d - p * kpq[:, None]) - s2 * (q - p),
            s2 * (-q * d - q * kqp[:, None]) - s1 * (p - q))
