"""Pair losses on MI355X: the class surface of abnet3/loss.py, HIP inside.

Mirrors (file:line relative to the reference checkout)
  LossBuilder   abnet3/loss.py:15-34
  coscos2       abnet3/loss.py:37-67
  cosmargin     abnet3/loss.py:70-105
  KLLoss        abnet3/loss.py:108-137
  weighted_loss_multi  abnet3/loss.py:140-182
forward(input1, input2, y) returns a 0-dim tensor with .backward(); the
arithmetic (cosine similarity with eps=1e-6 or the two KL divergences, per-label
transform, sum, /N) and its gradient run fused in one kernel (abn_pair_loss).
InfoNCELoss (not in the reference) is the in-batch contrastive loss over the same surface: forward(input1, input2, y,
groups=None); its B x B similarities never reach memory (abnt_nce_loss, csrc/nce.hip).
CorrespondenceLoss (not in the reference either) is the reconstruction loss of model.CorrespondenceAutoencoder:
forward(recon1, recon2, input1, input2, y), loss and gradient from one entry (abnr_recon_loss, csrc/recon.hip).
SoftDTWLoss (not in the reference either) is a loss over word PAIRS, not frame pairs: forward(e, off1, n1, off2, n2, y) over
the embedded rows of both words of every pair; the alignment is soft-DTW's and moves with the weights (abnq_softdtw_forward /
abnq_softdtw_backward, csrc/softdtw.hip, through abnet3_amd/softdtw.py).
"""
import torch
import torch.nn as nn

from . import _lib


_UNIT = {}        # device -> 0-dim tensor holding 1.0, never written again


def unit_grad(device):
    """The gradient seed d loss / d loss = 1 as a cached device tensor.  A trainer
    that starts backward with it (torch.autograd.backward(loss, unit_grad(dev)))
    saves autograd's ones_like fill, and the pair loss recognises it by address and
    hands its stored gradient back without the multiply by 1."""
    key = torch.device(device)
    if key.type == 'cuda' and key.index is None:
        key = torch.device('cuda', torch.cuda.current_device())
    t = _UNIT.get(key)
    if t is None:
        if key.type == 'cuda' and not torch.cuda.is_current_stream_capturing():
            # built once, read by whichever stream calls next: a blocking upload, complete before this returns (a fill
            # kernel would be ordered on the building stream alone)
            t = torch.ones((), dtype=torch.float32).to(key)
        else:
            t = torch.ones((), dtype=torch.float32, device=key)
        _UNIT[key] = t
    return t


_WS = {}          # (device index, stream) -> zero-initialised scratch (partial sums + ticket counter)
# a failed launch may leave a ticket counter non-zero: the cached buffers are dropped (and zeroed afresh on the next call)
_lib._ON_ERROR.append(_WS.clear)


def _scratch(nbytes, device):
    """abn_pair_loss's scratch: its ticket counter has to be zero before the first call and is
    left zero by every call, so one buffer per (device, stream) is zeroed once and reused."""
    if torch.cuda.is_current_stream_capturing():
        # inside a hipGraph capture: a buffer of the graph's own pool, zeroed by a captured memset
        return torch.zeros(max(int(nbytes), 4096), dtype=torch.uint8, device=device)
    key = (device.index, torch.cuda.current_stream(device).cuda_stream)
    ws = _WS.get(key)
    if ws is None or ws.numel() < nbytes:
        ws = _WS[key] = torch.zeros(max(int(nbytes), 4096), dtype=torch.uint8, device=device)
    return ws


def _pair_loss_raw(e1, e2, y, kind, margin, avg, need_grad, act=None, masks=None):
    """abn_pair_loss: (0-dim loss, [2, B, D] gradient of the loss w.r.t. (e1, e2) or None).
    With `act` (the activation that produced e1 / e2) the gradient is taken w.r.t. the
    pre-activations instead (abn_pair_loss_dz; `masks` = the output layer's dropout
    multipliers for the two towers, or None).  act = 'softmax' (KLLoss only): e1 / e2 are
    the logits of a softmax head and the gradient is d loss / d logits."""
    lib = _lib.load()
    _lib.require_device(e1, e2, y)
    if e1.dtype != torch.float32 or e2.dtype != torch.float32:
        raise TypeError('abnet3_amd: embeddings must be float32')
    if y.dtype not in _lib.Y_DTYPE:
        raise TypeError('abnet3_amd: unsupported label dtype %s' % y.dtype)
    B, D = e1.shape
    if y.numel() != B:
        raise ValueError('abnet3_amd: %d labels for %d pairs' % (y.numel(), B))
    e1, e2, y = e1.contiguous(), e2.contiguous(), y.contiguous()
    loss = torch.empty((), dtype=torch.float32, device=e1.device)
    de = torch.empty(2, B, D, dtype=torch.float32, device=e1.device) if need_grad else None
    ws = _scratch(lib.abn_pair_loss_ws_bytes(B), e1.device)
    if act is not None:
        m1, m2 = masks if masks is not None else (None, None)
        _lib.check(lib.abn_pair_loss_dz(
            _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], B, D,
            _lib.LOSS[kind], float(margin), int(bool(avg)),
            _lib.ACT_SOFTMAX if act == 'softmax' else _lib.ACT[act], _lib.ptr(m1), _lib.ptr(m2),
            _lib.ptr(loss), _lib.ptr(de[0]), _lib.ptr(de[1]), _lib.ptr(ws), _lib.stream()),
            'abn_pair_loss_dz')
        return loss, de
    _lib.check(lib.abn_pair_loss(
        _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], B, D,
        _lib.LOSS[kind], float(margin), int(bool(avg)), _lib.ptr(loss),
        _lib.ptr(de[0]) if need_grad else None,
        _lib.ptr(de[1]) if need_grad else None, _lib.ptr(ws), _lib.stream()),
        'abn_pair_loss')
    return loss, de


class _PairLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e1, e2, y, kind, margin, avg):
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, ctx.de = _pair_loss_raw(e1, e2, y, kind, margin, avg, need_grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        de = ctx.de
        if de is None:
            return None, None, None, None, None, None
        # d loss / d e was produced with the forward; chain the incoming scalar
        # (unless it is the cached unit seed, identified by its address)
        unit = _UNIT.get(g.device)
        if unit is None or g.data_ptr() != unit.data_ptr():
            de = de * g
        return de[0], de[1], None, None, None, None


class LossBuilder(nn.Module):
    """Generic Loss class for ABnet3 (abnet3/loss.py:15-34)."""

    def __init__(self, *args, **kwargs):
        super(LossBuilder, self).__init__(*args, **kwargs)

    def forward(self, *args, **kwargs):
        raise NotImplementedError('Unimplemented forward for class:',
                                  self.__class__.__name__)

    def whoami(self, *args, **kwargs):
        return {'params': self.__dict__, 'class_name': self.__class__.__name__}


def _pair_loss(input1, input2, y, kind, margin, avg):
    assert input1.size() == input2.size(), 'Input not the same size'
    return _PairLossFunction.apply(input1.contiguous(), input2.contiguous(),
                                   y.contiguous(), kind, margin, avg)


class coscos2(LossBuilder):
    """coscos2 Loss function (abnet3/loss.py:37-67)."""

    def __init__(self, avg=True, *args, **kwargs):
        super(coscos2, self).__init__(*args, **kwargs)
        self.avg = avg

    def forward(self, input1, input2, y):
        return _pair_loss(input1, input2, y, 'coscos2', 0.0, self.avg)

    def value_and_grad(self, input1, input2, y):
        """(loss, [2, B, D] gradient w.r.t. (input1, input2)) without autograd: what
        forward(...).backward() yields, for a trainer that drives the kernels itself."""
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'coscos2', 0.0, self.avg, True)

    def value_and_dz(self, input1, input2, y, act, masks=None):
        """(loss, [2, B, D] gradient w.r.t. the PRE-activations of the layer that produced the
        inputs through `act`): the loss gradient and the output layer's activation derivative
        in one launch."""
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'coscos2', 0.0, self.avg, True, act=act, masks=masks)


class cosmargin(LossBuilder):
    """cosmargin Loss function (abnet3/loss.py:70-105); margin in [0, 1]."""

    def __init__(self, avg=True, margin=0.5, *args, **kwargs):
        super(cosmargin, self).__init__(*args, **kwargs)
        self.margin = margin
        self.avg = avg
        assert (margin >= 0 and margin <= 1)

    def forward(self, input1, input2, y, avg=True):
        # like the reference, the `avg` ARGUMENT is ignored (loss.py:103)
        return _pair_loss(input1, input2, y, 'cosmargin', self.margin, self.avg)

    def value_and_grad(self, input1, input2, y):
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'cosmargin', self.margin, self.avg, True)

    def value_and_dz(self, input1, input2, y, act, masks=None):
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'cosmargin', self.margin, self.avg, True, act=act, masks=masks)


class KLLoss(LossBuilder):
    """The contrastive KL loss (abnet3/loss.py:108-137) of two probability rows P, Q:
    KL(P, Q) when they embed the same phoneme, max(0, margin - KL(P, Q)) when not, for both
    KL(P||Q) and KL(Q||P) -- nn.HingeEmbeddingLoss(margin, size_average=avg) of each, summed.
    Labels other than +-1 take KL + max(0, margin - KL), as the hinge loss does.  The margin
    has no range check; like the reference, forward's `avg` ARGUMENT is ignored."""

    def __init__(self, margin=1, avg=True, *args, **kwargs):
        super(KLLoss, self).__init__(*args, **kwargs)
        self.margin = margin
        self.avg = avg

    def forward(self, input1, input2, y, avg=True):
        return _pair_loss(input1, input2, y, 'KLLoss', self.margin, self.avg)

    def value_and_grad(self, input1, input2, y):
        """(loss, [2, B, D] gradient w.r.t. the probability rows (input1, input2))."""
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'KLLoss', self.margin, self.avg, True)

    def value_and_dz(self, input1, input2, y, act, masks=None):
        """act = 'softmax': input1 / input2 are LOGITS, the loss is that of their row softmaxes
        (nn.Softmax, a 'softmax' last_non_linearity) and the gradient is w.r.t. the logits --
        softmax, loss and gradient in one launch.  Other acts: as coscos2.value_and_dz, on
        probability rows act(z)."""
        assert input1.size() == input2.size(), 'Input not the same size'
        return _pair_loss_raw(input1, input2, y, 'KLLoss', self.margin, self.avg, True, act=act, masks=masks)


def _nce_raw(e1, e2, y, groups, tau, avg, need_grad):
    """abnt_nce_loss: (0-dim loss, [2, B, D] gradient of the loss w.r.t. (e1, e2) or None)."""
    lib = _lib.load()
    _lib.require_device(e1, e2, y)
    if e1.dtype != torch.float32 or e2.dtype != torch.float32:
        raise TypeError('abnet3_amd: embeddings must be float32')
    if y.dtype not in _lib.Y_DTYPE:
        raise TypeError('abnet3_amd: unsupported label dtype %s' % y.dtype)
    if e1.dim() != 2 or e1.size() != e2.size():
        raise ValueError('abnet3_amd: InfoNCELoss takes two [B, D] inputs of one shape')
    B, D = e1.shape
    if y.numel() != B:
        raise ValueError('abnet3_amd: %d labels for %d pairs' % (y.numel(), B))
    if D > lib.abnt_nce_max_d():
        raise ValueError('abnet3_amd: InfoNCELoss takes embeddings of at most %d columns (abnt_nce_max_d), got %d'
                         % (lib.abnt_nce_max_d(), D))
    if groups is not None:
        _lib.require_device(groups)
        if groups.numel() != B:
            raise ValueError('abnet3_amd: %d groups for %d pairs' % (groups.numel(), B))
        groups = groups.to(torch.int32).contiguous()
    e1, e2, y = e1.contiguous(), e2.contiguous(), y.contiguous()
    need = lib.abnt_nce_ws_bytes(B, D)
    if need < 0:
        _lib.check(_lib.E_UNSUPPORTED, 'abnt_nce_ws_bytes')
    loss = torch.empty((), dtype=torch.float32, device=e1.device)
    de = torch.empty(2, B, D, dtype=torch.float32, device=e1.device) if need_grad else None
    ws = torch.empty(need, dtype=torch.uint8, device=e1.device)          # need not be cleared
    _lib.check(lib.abnt_nce_loss(
        _lib.ptr(e1), _lib.ptr(e2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype], _lib.ptr(groups), B, D, float(tau),
        int(bool(avg)), _lib.ptr(loss), None, _lib.ptr(de[0]) if need_grad else None,
        _lib.ptr(de[1]) if need_grad else None, _lib.ptr(ws), _lib.stream()), 'abnt_nce_loss')
    return loss, de


class _NceFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e1, e2, y, groups, tau, avg):
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, ctx.de = _nce_raw(e1, e2, y, groups, tau, avg, need_grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        de = ctx.de
        if de is None:
            return None, None, None, None, None, None
        unit = _UNIT.get(g.device)                    # (the cached unit seed: _PairLossFunction.backward)
        if unit is None or g.data_ptr() != unit.data_ptr():
            de = de * g
        return de[0], de[1], None, None, None, None


class InfoNCELoss(LossBuilder):
    """The in-batch contrastive loss (InfoNCE / NT-Xent) of B pairs: row i of input1 and row i of input2 are a positive, every
    other row of the batch is a negative -- no 'different' pairs are sampled.  Not part of the reference; for the pair
    sources that yield positives only (mined pairs, cluster sampling, temporal coherence).

    With a^_i = input1_i / max(|input1_i|, 1e-6), b^_j likewise, s[i][j] = <a^_i, b^_j>, r[i] = (y[i] == 1), n = sum r:
        la[i] = log sum_j exp(s[i][j] / temperature)      (a^_i against every b^_j)
        lb[j] = log sum_i exp(s[i][j] / temperature)      (b^_j against every a^_i)
        loss  = sum_i r[i] ((la[i] + lb[i]) / 2 - s[i][i] / temperature),  divided by n when avg.
    A row with y != 1 is no anchor, but its two vectors stay among everyone's candidates.  n = 0 gives loss 0 and zero
    gradients for either avg -- deliberately NOT the NaN an empty batch gives the cosine losses: a batch without a positive
    is an ordinary event for a sampled loader and must not poison the weights.  `groups` ([B] integers, optional) excludes
    the cells (i, j), j != i, with groups[i] == groups[j] from both sums: frames of one word pair are near-duplicates and
    would be false negatives.  No loader delivers groups yet.

    temperature = 0.1 is a common starting point and is NOT tuned on speech.  Loss and both gradients come from one C
    entry (abnt_nce_loss, csrc/nce.hip): the B x B similarities never reach memory.  Under data parallelism the negatives
    are those of the rank's own batch; nothing is gathered across ranks.  Trains through autograd (the trainer's direct and
    planned steps do not know this loss and step aside)."""

    def __init__(self, temperature=0.1, avg=True, *args, **kwargs):
        super(InfoNCELoss, self).__init__(*args, **kwargs)
        if not (float(temperature) > 0.0) or float(temperature) == float('inf'):
            raise ValueError('abnet3_amd: InfoNCELoss temperature = %r must be finite and > 0' % (temperature,))
        self.temperature = temperature
        self.avg = avg

    def forward(self, input1, input2, y, groups=None):
        assert input1.size() == input2.size(), 'Input not the same size'
        return _NceFunction.apply(input1.contiguous(), input2.contiguous(), y.contiguous(), groups, self.temperature, self.avg)

    def value_and_grad(self, input1, input2, y, groups=None):
        """(loss, [2, B, D] gradient w.r.t. (input1, input2)) without autograd."""
        assert input1.size() == input2.size(), 'Input not the same size'
        return _nce_raw(input1, input2, y, groups, self.temperature, self.avg, True)


RECON_MODE = {'correspondence': 0, 'autoencoder': 1}


def _recon_raw(r1, r2, x1, x2, y, mode, symmetric, avg, need_grad):
    """abnr_recon_loss: (0-dim loss, [2, B, D] gradient of the loss w.r.t. (r1, r2) or None)."""
    if mode not in RECON_MODE:
        raise ValueError("abnet3_amd: CorrespondenceLoss mode = %r, supported 'correspondence', 'autoencoder'" % (mode,))
    for what, t in (('recon1', r1), ('recon2', r2), ('input1', x1), ('input2', x2)):
        if not isinstance(t, torch.Tensor):
            raise TypeError('abnet3_amd: CorrespondenceLoss %s must be a tensor, not %s' % (what, type(t).__name__))
        if t.dtype != torch.float32:
            raise TypeError('abnet3_amd: CorrespondenceLoss %s must be float32, not %s' % (what, t.dtype))
        if t.dim() != 2 or t.size() != r1.size():
            raise ValueError('abnet3_amd: CorrespondenceLoss takes four [B, D] tensors of one shape (%s is %s, recon1 %s)'
                             % (what, tuple(t.shape), tuple(r1.shape)))
    if mode == 'autoencoder':
        y = None                                   # (every row counts: the labels are not read)
    elif not isinstance(y, torch.Tensor) or y.dtype not in _lib.Y_DTYPE:
        raise TypeError('abnet3_amd: unsupported label dtype %s' % (y.dtype if isinstance(y, torch.Tensor) else type(y).__name__))
    B, D = r1.shape
    if y is not None and (y.dim() != 1 or y.numel() != B):
        raise ValueError('abnet3_amd: %s labels for %d pairs' % (tuple(y.shape), B))
    lib = _lib.load()
    r1, r2, x1, x2 = r1.contiguous(), r2.contiguous(), x1.contiguous(), x2.contiguous()
    y = y.contiguous() if y is not None else None
    _lib.require_device(r1, r2, x1, x2, y)
    if D > lib.abnr_recon_max_d():
        raise ValueError('abnet3_amd: CorrespondenceLoss takes rows of at most %d columns (abnr_recon_max_d), got %d'
                         % (lib.abnr_recon_max_d(), D))
    need = lib.abnr_recon_ws_bytes(B, D)
    if need < 0:
        _lib.check(_lib.E_UNSUPPORTED, 'abnr_recon_ws_bytes')
    loss = torch.empty((), dtype=torch.float32, device=r1.device)
    dr = torch.empty(2, B, D, dtype=torch.float32, device=r1.device) if need_grad else None
    ws = torch.empty(need, dtype=torch.uint8, device=r1.device)          # need not be cleared
    _lib.check(lib.abnr_recon_loss(
        _lib.ptr(r1), _lib.ptr(r2), _lib.ptr(x1), _lib.ptr(x2), _lib.ptr(y), _lib.Y_DTYPE[y.dtype] if y is not None else 0, B, D,
        RECON_MODE[mode], int(bool(symmetric)), int(bool(avg)), _lib.ptr(loss), None, _lib.ptr(dr[0]) if need_grad else None,
        _lib.ptr(dr[1]) if need_grad else None, _lib.ptr(ws), _lib.stream()), 'abnr_recon_loss')
    return loss, dr


class _ReconFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, r1, r2, x1, x2, y, mode, symmetric, avg):
        need_grad = ctx.needs_input_grad[0] or ctx.needs_input_grad[1]
        loss, ctx.dr = _recon_raw(r1, r2, x1, x2, y, mode, symmetric, avg, need_grad)
        return loss

    @staticmethod
    def backward(ctx, g):
        dr = ctx.dr
        if dr is None:
            return None, None, None, None, None, None, None, None
        unit = _UNIT.get(g.device)                    # (the cached unit seed: _PairLossFunction.backward)
        if unit is None or g.data_ptr() != unit.data_ptr():
            dr = dr * g
        return dr[0], dr[1], None, None, None, None, None, None


class CorrespondenceLoss(LossBuilder):
    """The reconstruction loss of the correspondence autoencoder (Kamper et al. 2015; not part of the reference):
    forward(recon1, recon2, input1, input2, y) with recon = network(input1, input2) of a CorrespondenceAutoencoder.

    With s = 1 if symmetric else 0:
        mode 'correspondence':  R = {i : y[i] == 1},  t[i] = |recon1[i] - input2[i]|^2 + s |recon2[i] - input1[i]|^2
                                (each tower reconstructs its aligned PARTNER; a 'different' row carries no target and no gradient)
        mode 'autoencoder':     R = every row, y is ignored,  t[i] = |recon1[i] - input1[i]|^2 + s |recon2[i] - input2[i]|^2
                                (the pretraining pass: each tower reconstructs its own input)
        loss = sum over R of t[i], divided by |R| D (1 + s) when avg: the mean squared error per reconstructed element.
    |R| = 0 gives loss 0 and zero gradients for either avg (InfoNCELoss's decision, for its reason: a batch without a 'same'
    pair is an ordinary event for a sampled loader).  `mode` may be reassigned between passes (TrainerCorrespondence.pretrain
    does).  Loss and both gradients come from one C entry (abnr_recon_loss, csrc/recon.hip), float64 inside, the same bits
    from call to call.  The inputs get no gradient.  Trains through autograd (the trainer's direct and planned steps do not
    know this loss and step aside).  Nothing here is tuned or measured on real speech."""

    def __init__(self, avg=True, symmetric=True, mode='correspondence', *args, **kwargs):
        super(CorrespondenceLoss, self).__init__(*args, **kwargs)
        if mode not in RECON_MODE:
            raise ValueError("abnet3_amd: CorrespondenceLoss mode = %r, supported 'correspondence', 'autoencoder'" % (mode,))
        self.avg = avg
        self.symmetric = symmetric
        self.mode = mode

    def forward(self, recon1, recon2, input1, input2, y=None):
        return _ReconFunction.apply(recon1, recon2, input1, input2, y, self.mode, self.symmetric, self.avg)

    def value_and_grad(self, recon1, recon2, input1, input2, y=None):
        """(loss, [2, B, D] gradient w.r.t. (recon1, recon2)) without autograd."""
        return _recon_raw(recon1, recon2, input1, input2, y, self.mode, self.symmetric, self.avg, True)


class SoftDTWLoss(LossBuilder):
    """A contrastive loss over WORD pairs under a differentiable alignment (soft-DTW, Cuturi & Blondel 2017; not part of the
    reference): forward(e, off1, n1, off2, n2, y).  e [R, D] holds the embedded frames of a batch; word pair p is the rows
    e[off1[p] : off1[p] + n1[p]] against e[off2[p] : off2[p] + n2[p]] (off*, n*: host sequences; within a side the pairs'
    row ranges must not overlap); y [P] on the device, "same" is y == 1.

    With value(x, y) the soft-DTW value over the cells 1 - cos(x_i, y_j) (softdtw.soft_dtw: include/abnet3_hip_next.h states
    the recurrence, tests/sdtw_np.py restates it):
        v_p  = value(x, y),  or with divergence:  value(x, y) - (value(x, x) + value(y, y)) / 2   (>= 0, 0 for x == y)
        s_p  = v_p / (n1[p] + n2[p]) when normalize, else v_p
        term = s_p where y[p] == 1,  max(0, margin - s_p) elsewhere
        loss = sum of the terms, divided by P when avg.  P == 0 gives 0.
    Unlike the frame-pair losses the alignment is not frozen: it is a function of the embeddings and moves with the weights.
    The sweeps run in the kernels; the arithmetic on the [P] vectors is plain torch, which also supplies the weights the
    backward kernel takes.  The divergence costs three soft_dtw calls.

    gamma = 0.1 and margin = 0.5 are UNTUNED: nothing has been measured on speech.  gamma -> 0 approaches the hard DTW cost
    (value <= hard cost <= value + gamma log(3) (n + m - 2)).  Trains through autograd (the trainer's direct and planned
    steps do not know this loss and step aside); single process."""

    def __init__(self, gamma=0.1, margin=0.5, normalize=True, divergence=False, avg=True, *args, **kwargs):
        super(SoftDTWLoss, self).__init__(*args, **kwargs)
        if not (float(gamma) > 0.0) or float(gamma) == float('inf'):
            raise ValueError('abnet3_amd: SoftDTWLoss gamma = %r must be finite and > 0' % (gamma,))
        self.gamma = gamma
        self.margin = margin
        self.normalize = normalize
        self.divergence = divergence
        self.avg = avg

    def check_batch(self, rows, off1, n1, off2, n2, y):
        """The columns as host arrays, after every check of a batch that needs no embedding: the columns' shapes, the row
        ranges (inside a table of `rows` rows, at least one row and at most softdtw.max_len() a side, no overlap within a
        side) and the labels.  A trainer calls it BEFORE the tower runs, so that a bad batch is refused before any launch."""
        from . import softdtw
        cols = softdtw.require_disjoint('SoftDTWLoss', off1, n1, off2, n2)
        softdtw.require_ranges('SoftDTWLoss', rows, *cols)
        _lib.require_tensor('SoftDTWLoss', 'y', y, tuple(_lib.Y_DTYPE), 1)
        if y.shape[0] != len(cols[1]):
            raise ValueError('abnet3_amd: SoftDTWLoss: %d labels for %d word pairs' % (y.shape[0], len(cols[1])))
        return cols

    def _check(self, e, off1, n1, off2, n2, y):
        _lib.require_tensor('SoftDTWLoss', 'e', e, torch.float32, 2)
        return self.check_batch(e.shape[0], off1, n1, off2, n2, y)

    def _terms(self, v, lens, y):
        """The pairs' terms [P] from their values."""
        s = v / lens if self.normalize else v
        same = y == 1
        return torch.where(same, s, torch.clamp(self.margin - s, min=0.0))

    def forward(self, e, off1, n1, off2, n2, y, checked=False):
        """checked=True: off1, n1, off2, n2 are what check_batch(e.shape[0], ..., y) returned for this very batch (a trainer
        that checked before its tower ran): the host checks are not repeated."""
        from .softdtw import soft_dtw
        if checked:
            _lib.require_tensor('SoftDTWLoss', 'e', e, torch.float32, 2)
        else:
            off1, n1, off2, n2 = self._check(e, off1, n1, off2, n2, y)
        v = soft_dtw(e, off1, n1, off2, n2, self.gamma, checked=True)
        if self.divergence:
            v = v - 0.5 * (soft_dtw(e, off1, n1, off1, n1, self.gamma, checked=True) +
                           soft_dtw(e, off2, n2, off2, n2, self.gamma, checked=True))
        P = len(n1)
        lens = torch.from_numpy((n1 + n2).astype('float32')).to(e.device) if self.normalize else None
        loss = self._terms(v, lens, y).sum()
        return loss / P if (self.avg and P > 0) else loss

    def value_and_grad(self, e, off1, n1, off2, n2, y):
        """(loss, [R, D] gradient w.r.t. e) without autograd."""
        from . import softdtw
        off1, n1, off2, n2 = self._check(e, off1, n1, off2, n2, y)
        P = len(n1)
        with torch.no_grad():
            calls = [(off1, n1, off2, n2, 1.0)]
            if self.divergence:
                calls += [(off1, n1, off1, n1, -0.5), (off2, n2, off2, n2, -0.5)]
            done = [softdtw.soft_dtw_batch(e, a, b, c, d, self.gamma, keep=True) + (f,) for a, b, c, d, f in calls]
            v = done[0][0]
            if self.divergence:
                v = v - 0.5 * (done[1][0] + done[2][0])
            lens = torch.from_numpy((n1 + n2).astype('float32')).to(e.device) if self.normalize else None
            s = v / lens if self.normalize else v
            same = y == 1
            scale = 1.0 / P if (self.avg and P > 0) else 1.0
            loss = self._terms(v, lens, y).sum() * scale
            w = torch.where(same, torch.ones_like(s), -(self.margin - s > 0).to(s.dtype)) * scale
            if self.normalize:
                w = w / lens
            de = None
            for value, handle, f in done:
                g1, g2 = softdtw.soft_dtw_backward(handle, (w * f).contiguous())
                de = softdtw.fold_blocks(handle, g1, g2, de)
        return loss, de


class weighted_loss_multi(LossBuilder):
    """Weighted loss for multi-task training based on two pair losses
    (abnet3/loss.py:140-182): weight*loss_spk + (1 - weight)*loss_phn.

    Parameters
    ----------
    loss_phn, loss_spk : abnet3_amd.loss functions (coscos2 / cosmargin / KLLoss; each
        sub-loss runs through autograd, a KLLoss on its probability form)
    weight : float
        variable between 0 and 1, to weight one or the other task.
    """

    def __init__(self, avg=True, loss_phn=None, loss_spk=None,
                 weight=0.5, *args, **kwargs):
        super(weighted_loss_multi, self).__init__(*args, **kwargs)
        assert type(weight) is float
        assert (weight >= 0 and weight <= 1)
        self.weight = weight
        self.avg = avg
        self.loss_phn = loss_phn
        self.loss_spk = loss_spk

    def forward(self, emb_spk1, emb_phn1, emb_spk2, emb_phn2,
                y_spk, y_phn):
        output_spk = self.loss_spk(emb_spk1, emb_spk2, y_spk)
        output_phn = self.loss_phn(emb_phn1, emb_phn2, y_phn)
        output = self.weight * output_spk + (1.0 - self.weight) * output_phn
        return output

