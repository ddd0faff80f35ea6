"""The correspondence autoencoder restated for the tests: CorrespondenceLoss and its gradients in float64 numpy with explicit
loops over the rows (abnet3_amd/loss.py states the definition, include/abnet3_hip_next.h the entry's), and a torch-CPU
evaluator of a CorrespondenceAutoencoder in float64 or float32 that calls deep copies of the network's OWN nn.Sequential
modules (p_dropout = 0: nn.Dropout is then the identity in either mode), with k optimizer steps of torch.optim on that copy."""
import copy

import numpy as np

MODES = ('correspondence', 'autoencoder')


def counted_rows(y, mode, B):
    """[B] bool: the rows of R.  'Same' is y == 1 whatever the dtype (2, 0, -1, 1.5: not same)."""
    if mode == 'autoencoder':
        return np.ones(B, dtype=bool)
    return np.array([float(v) == 1.0 for v in np.asarray(y).reshape(-1)], dtype=bool)


def scale_of(n, D, symmetric, avg):
    if n == 0:
        return 0.0
    return 1.0 / (n * D * (2 if symmetric else 1)) if avg else 1.0


def recon_loss(r1, r2, x1, x2, y, mode='correspondence', symmetric=True, avg=True):
    """(loss, terms [B], dr1 [B][D], dr2 [B][D]) in float64, row by row."""
    assert mode in MODES
    r1, r2, x1, x2 = (np.asarray(a, dtype=np.float64) for a in (r1, r2, x1, x2))
    B, D = r1.shape
    counted = counted_rows(y, mode, B)
    t1, t2 = (x2, x1) if mode == 'correspondence' else (x1, x2)
    c = scale_of(int(counted.sum()), D, symmetric, avg)
    terms, dr1, dr2 = np.zeros(B), np.zeros((B, D)), np.zeros((B, D))
    total = 0.0
    for i in range(B):
        if not counted[i]:
            continue
        a = r1[i] - t1[i]
        terms[i] = float(np.dot(a, a))
        dr1[i] = 2.0 * c * a
        if symmetric:
            b = r2[i] - t2[i]
            terms[i] += float(np.dot(b, b))
            dr2[i] = 2.0 * c * b
        total += terms[i]
    return c * total, terms, dr1, dr2


def brute_loss(r1, r2, x1, x2, y, mode, symmetric, avg):
    """The definition element by element, nothing shared with recon_loss but the rule for 'same'."""
    B, D = np.shape(r1)
    total, n, s = 0.0, 0, (1.0 if symmetric else 0.0)
    for i in range(B):
        if mode == 'correspondence' and float(np.asarray(y).reshape(-1)[i]) != 1.0:
            continue
        n += 1
        for d in range(D):
            if mode == 'correspondence':
                total += (float(r1[i][d]) - float(x2[i][d])) ** 2 + s * (float(r2[i][d]) - float(x1[i][d])) ** 2
            else:
                total += (float(r1[i][d]) - float(x1[i][d])) ** 2 + s * (float(r2[i][d]) - float(x2[i][d])) ** 2
    if avg and n:
        total /= n * D * (2 if symmetric else 1)
    return total


def torch_loss(r1, r2, x1, x2, y, mode, symmetric, avg):
    """The same loss from torch.nn.functional.mse_loss on the masked rows (any dtype; differentiable in r1, r2)."""
    import torch
    import torch.nn.functional as F
    B, D = r1.shape
    keep = torch.ones(B, dtype=torch.bool) if mode == 'autoencoder' else (y.reshape(-1).double() == 1.0)
    t1, t2 = (x2, x1) if mode == 'correspondence' else (x1, x2)
    n = int(keep.sum())
    if n == 0:
        return (r1.sum() + r2.sum()) * 0.0
    total = F.mse_loss(r1[keep], t1[keep], reduction='sum')
    if symmetric:
        total = total + F.mse_loss(r2[keep], t2[keep], reduction='sum')
    return total / (n * D * (2 if symmetric else 1)) if avg else total


def draw(rng, B, D, labels=(1, -1, 0, 2), y_dtype=np.int64):
    """Four [B][D] float32 tables and [B] labels from `labels`."""
    r1, r2, x1, x2 = (rng.standard_normal((B, D)).astype(np.float32) for _ in range(4))
    y = rng.choice(np.asarray(labels), B).astype(y_dtype)
    return r1, r2, x1, x2, y


# ---- the network on the CPU ---------------------------------------------------------------------------------------------
ENCODER = ('input_emb', 'hidden_layers', 'output_layer')


def pre_bn_bias(k, batch_norm):
    """A Linear bias in front of a BatchNorm1d: mathematically without effect, its gradient is rounding noise on every side."""
    if not batch_norm or not k.endswith('.bias') or k.startswith('recon_layer'):
        return False
    return int(k.split('.')[1]) % 4 == 0


class CpuCae(object):
    """Deep copies of a CorrespondenceAutoencoder's own modules on the CPU in `dtype`."""

    def __init__(self, net, dtype):
        import torch
        assert float(net.p_dropout) == 0.0
        self.dtype = dtype
        self.names = ENCODER + ('decoder_layers', 'recon_layer')
        self.mods = torch.nn.ModuleDict({n: copy.deepcopy(getattr(net, n)).cpu().to(dtype) for n in self.names})
        self.mods.train(net.training)

    def train(self, mode=True):
        self.mods.train(mode)
        return self

    def encode(self, x):
        for n in ENCODER:
            x = self.mods[n](x)
        return x

    def decode(self, h):
        return self.mods['recon_layer'](self.mods['decoder_layers'](h))

    def forward_once(self, x):
        return self.encode(x.to(self.dtype))

    def reconstruct(self, x):
        return self.decode(self.encode(x.to(self.dtype)))

    def forward(self, x1, x2):
        return self.reconstruct(x1), self.reconstruct(x2)         # two tower calls: BatchNorm statistics per call

    def named_parameters(self):
        return {k: p for k, p in self.mods.named_parameters()}

    def state(self):
        return {k: v.detach().double().numpy().copy() for k, v in self.mods.state_dict().items()}

    def loss(self, batch, mode, symmetric, avg):
        x1, x2, y = batch
        x1, x2 = x1.to(self.dtype), x2.to(self.dtype)
        r1, r2 = self.forward(x1, x2)
        return torch_loss(r1, r2, x1, x2, y, mode, symmetric, avg)

    def run_steps(self, batches, k, make_optimizer, mode='correspondence', symmetric=True, avg=True):
        """k steps of the reference's five statements on this copy: (losses, gradients of the FIRST step, state after)."""
        opt = make_optimizer(self.mods.parameters())
        losses, first = [], None
        for s in range(k):
            lv = self.loss(batches[s % len(batches)], mode, symmetric, avg)
            opt.zero_grad()
            lv.backward()
            if s == 0:
                first = {n: p.grad.detach().double().numpy().copy() for n, p in self.mods.named_parameters()}
            opt.step()
            losses.append(float(lv.detach()))
        return losses, first, self.state()


def planted_corpus(rng, n, dim=40, sub=8, noise=0.05, p_same=0.5):
    """x1 on a random `sub`-dimensional subspace of `dim` dimensions; x2 = x1 + small noise on a 'same' row (y = 1), an
    unrelated point of the subspace on a 'different' one (y = -1)."""
    basis = rng.standard_normal((sub, dim)) / np.sqrt(sub)
    x1 = rng.standard_normal((n, sub)) @ basis
    other = rng.standard_normal((n, sub)) @ basis
    y = np.where(rng.random(n) < p_same, 1, -1).astype(np.int64)
    x2 = np.where((y == 1)[:, None], x1 + noise * rng.standard_normal((n, dim)), other)
    return x1.astype(np.float32), x2.astype(np.float32), y
