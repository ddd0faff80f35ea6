"""Batched soft-DTW over cosine cells on MI355X (Cuturi & Blondel 2017; not part of the reference): the value of a
differentiable alignment between two runs of rows of one table, and its gradient with respect to the rows.

    soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=False) -> (value [P], handle)       abnq_softdtw_forward
    soft_dtw_backward(handle, w) -> (g1 [sum n1, D], g2 [sum n2, D])                        abnq_softdtw_backward
    soft_dtw(e, off1, n1, off2, n2, gamma) -> value [P]                                     the two behind autograd

Problem p is x = e[off1[p] : off1[p] + n1[p]] against y = e[off2[p] : off2[p] + n2[p]]; the offsets and lengths are HOST
sequences (as in abx.dtw_cost_batch), uploaded in one copy per call.  include/abnet3_hip_next.h (section abnq_) states the
definition, tests/sdtw_np.py restates it in float64, csrc/softdtw.hip holds the kernels.  The entries read the problem table
back to refuse a bad one before any launch, so a call waits for the stream once: not for graph capture."""
import ctypes as C

import numpy as np
import torch

from . import _lib


def max_len():
    """Most rows of either side of a problem (abnq_softdtw_max_len)."""
    return int(_lib.load().abnq_softdtw_max_len())


def max_d():
    """Most columns of the table (abnq_softdtw_max_d)."""
    return int(_lib.load().abnq_softdtw_max_d())


class Handle(object):
    """What soft_dtw_backward needs of a soft_dtw_batch(keep=True) call: the table, the problem arrays on the device and the
    workspace the forward left."""

    def __init__(self, e, cols, dev, gamma, ws, keep):
        self.e, self.cols, self.dev, self.gamma, self.ws, self.keep = e, cols, dev, gamma, ws, keep
        self.P = len(cols[1])
        self.rows1, self.rows2 = int(cols[1].sum()), int(cols[3].sum())


def _columns(who, off1, n1, off2, n2):
    """The four columns as contiguous host arrays (int64 offsets, int32 lengths); ValueError for anything else."""
    try:
        off1, off2 = (np.ascontiguousarray(a, dtype=np.int64) for a in (off1, off2))
        n1, n2 = (np.ascontiguousarray(a, dtype=np.int32) for a in (n1, n2))
    except (TypeError, ValueError) as err:
        raise ValueError('%s: off1, n1, off2, n2 must be sequences of integers (%s)' % (who, err))
    if any(a.ndim != 1 for a in (off1, n1, off2, n2)) or not (len(off1) == len(off2) == len(n1) == len(n2)):
        raise ValueError('%s: off1, n1, off2, n2 must be 1-d and of one length' % who)
    return off1, n1, off2, n2


def require_ranges(who, rows, off1, n1, off2, n2):
    """ValueError for an empty or too long side, or a run outside a table of `rows` rows (columns as _columns returns them)."""
    if len(n1):
        cap = max_len()
        if n1.min() < 1 or n2.min() < 1:
            raise ValueError('%s: every side needs at least one row' % who)
        if n1.max() > cap or n2.max() > cap:
            raise ValueError('%s: a side has %d rows, at most %d are taken (softdtw.max_len())' % (who, max(n1.max(), n2.max()), cap))
        if off1.min() < 0 or off2.min() < 0 or (off1 + n1).max() > rows or (off2 + n2).max() > rows:
            raise ValueError('%s: a problem reads outside the table of %d rows' % (who, rows))


def _problem_table(who, rows, off1, n1, off2, n2, device):
    """The four columns as (host arrays, device tensors): one upload.  ValueError for columns of different lengths, a rank
    other than 1, an empty or too long side, or a run outside the table."""
    off1, n1, off2, n2 = _columns(who, off1, n1, off2, n2)
    require_ranges(who, rows, off1, n1, off2, n2)
    P = len(n1)
    buf = np.empty(3 * P, dtype=np.int64)
    buf[:P], buf[P:2 * P] = off1, off2
    lens = buf[2 * P:].view(np.int32)
    lens[:P], lens[P:] = n1, n2
    if P == 0:
        none64, none32 = torch.zeros(0, dtype=torch.int64, device=device), torch.zeros(0, dtype=torch.int32, device=device)
        return (off1, n1, off2, n2), (none64, none32, none64, none32)
    d = torch.from_numpy(buf).to(device)
    dl = d[2 * P:].view(torch.int32)
    return (off1, n1, off2, n2), (d[:P], dl[:P], d[P:2 * P], dl[P:])


def _check_gamma(who, gamma):
    gamma = float(gamma)
    if not (gamma > 0.0) or gamma == float('inf') or not np.isfinite(np.float32(gamma)) or not np.float32(gamma) > 0:
        raise ValueError('%s: gamma = %r must be finite and > 0' % (who, gamma))
    return gamma


def soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=False):
    """(value [P] float32 on the device, Handle).  With keep the handle can be given to soft_dtw_backward; without, the
    workspace is smaller and nothing is stored for a backward (inference, a dev loss)."""
    who = 'soft_dtw_batch'
    _lib.require_tensor(who, 'e', e, torch.float32, 2)
    gamma = _check_gamma(who, gamma)
    lib = _lib.load()
    R, D = e.shape
    if D < 1 or D > max_d():
        raise ValueError('%s: the table has %d columns, 1 .. %d are taken (softdtw.max_d())' % (who, D, max_d()))
    cols, dev = _problem_table(who, R, off1, n1, off2, n2, e.device)
    P = len(cols[1])
    value = torch.empty(P, dtype=torch.float32, device=e.device)
    if P == 0:
        return value, Handle(e, cols, dev, gamma, None, bool(keep))
    need = lib.abnq_softdtw_ws_bytes(cols[1].ctypes.data_as(C.c_void_p), cols[3].ctypes.data_as(C.c_void_p), P, D, int(bool(keep)))
    if need < 0:
        _lib.check(_lib.E_UNSUPPORTED, 'abnq_softdtw_ws_bytes')
    ws = torch.empty(need, dtype=torch.uint8, device=e.device)          # need not be cleared
    _lib.check(lib.abnq_softdtw_forward(_lib.ptr(e), R, D, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]),
                                        P, gamma, _lib.ptr(value), _lib.ptr(ws), need, int(bool(keep)), _lib.stream()),
               'abnq_softdtw_forward')
    return value, Handle(e, cols, dev, gamma, ws if keep else None, bool(keep))


def soft_dtw_backward(handle, w):
    """(g1 [sum n1, D], g2 [sum n2, D]): the gradients of sum_p w[p] value[p] with respect to the rows of side 1 and of side
    2, as blocks in problem order (problem p's side-1 rows start at sum(n1[:p])).  w [P] on the device, any floating dtype or
    layout (it is converted to contiguous float32)."""
    who = 'soft_dtw_backward'
    if not isinstance(handle, Handle):
        raise ValueError('%s: the handle of a soft_dtw_batch call is needed, not %s' % (who, type(handle).__name__))
    if not handle.keep:
        raise ValueError('%s: the forward ran with keep=False: nothing was stored for a backward' % who)
    if not isinstance(w, torch.Tensor) or w.dim() != 1 or not w.dtype.is_floating_point or w.shape[0] != handle.P:
        raise ValueError('%s: w must be a 1-d floating-point tensor of %d weights, not %s' % (
            who, handle.P, '%s %s' % (tuple(w.shape), w.dtype) if isinstance(w, torch.Tensor) else type(w).__name__))
    e, dev = handle.e, handle.dev
    if w.device != e.device:
        raise _lib.HipLibraryError('%s: w is on %s, the table on %s' % (who, w.device, e.device))
    w = w.to(torch.float32).contiguous()                     # (the forward has run: a view or a wider dtype is converted, not refused)
    _lib.require_tensor(who, 'w', w, torch.float32, 1)
    R, D = e.shape
    g1 = torch.empty(handle.rows1, D, dtype=torch.float32, device=e.device)
    g2 = torch.empty(handle.rows2, D, dtype=torch.float32, device=e.device)
    if handle.P == 0:
        return g1, g2
    _lib.check(_lib.load().abnq_softdtw_backward(
        _lib.ptr(e), R, D, _lib.ptr(dev[0]), _lib.ptr(dev[1]), _lib.ptr(dev[2]), _lib.ptr(dev[3]), handle.P, handle.gamma,
        _lib.ptr(w), _lib.ptr(g1), _lib.ptr(g2), _lib.ptr(handle.ws), handle.ws.numel(), _lib.stream()), 'abnq_softdtw_backward')
    return g1, g2


def _block_rows(off, n):
    """The table rows of one side's blocks, in block order (host int64)."""
    total = int(n.sum())
    if total == 0:
        return np.zeros(0, dtype=np.int64)
    starts = np.cumsum(n, dtype=np.int64) - n
    return np.repeat(off - starts, n) + np.arange(total, dtype=np.int64)


def _require_disjoint(who, side, off, n):
    """ValueError when two problems' row ranges of one side overlap: the fold of the gradient blocks is an index_add_ whose
    indices must be unique for its result to have one order."""
    order = np.argsort(off, kind='stable')
    o, l = off[order], n[order]
    if len(o) > 1 and ((o[:-1] + l[:-1]) > o[1:]).any():
        k = int(np.flatnonzero((o[:-1] + l[:-1]) > o[1:])[0])
        raise ValueError('%s: the rows of problems %d and %d overlap on side %d; within a side the problems\' row ranges must be '
                         'disjoint (side 1 and side 2 may coincide)' % (who, int(order[k]), int(order[k + 1]), side))


def fold_blocks(handle, g1, g2, de=None):
    """de [R, D] (zeros unless given) += the blocks of soft_dtw_backward at their table rows: two ordered index_add_ calls,
    the indices unique within each when the side's row ranges are disjoint, so every row of de receives at most one block
    row per call and the sum has one order."""
    e = handle.e
    off1, n1, off2, n2 = handle.cols
    rows = np.concatenate([_block_rows(off1, n1), _block_rows(off2, n2)])
    idx = torch.from_numpy(rows).to(e.device)               # one upload for both sides
    if de is None:
        de = torch.zeros_like(e)
    de.index_add_(0, idx[:handle.rows1], g1)
    de.index_add_(0, idx[handle.rows1:], g2)
    return de


def require_disjoint(who, off1, n1, off2, n2):
    """The columns as host arrays, after the check soft_dtw makes: no two problems' row ranges overlap within a side."""
    off1, n1, off2, n2 = _columns(who, off1, n1, off2, n2)
    _require_disjoint(who, 1, off1, n1)
    _require_disjoint(who, 2, off2, n2)
    return off1, n1, off2, n2


class _SoftDtwFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, e, off1, n1, off2, n2, gamma, checked):
        need = ctx.needs_input_grad[0]
        if not checked:
            off1, n1, off2, n2 = require_disjoint('soft_dtw', off1, n1, off2, n2)
        value, handle = soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=need)
        ctx.handle = handle if need else None
        if need:
            ctx.save_for_backward(e)         # the backward reads the rows again: autograd refuses an e changed in place since
        return value

    @staticmethod
    def backward(ctx, g):
        handle = ctx.handle
        if handle is None:
            return None, None, None, None, None, None, None
        e, = ctx.saved_tensors               # (raises if e was modified in place after the forward)
        assert e.data_ptr() == handle.e.data_ptr()
        g1, g2 = soft_dtw_backward(handle, g)
        de = fold_blocks(handle, g1, g2)
        return de, None, None, None, None, None, None


def soft_dtw(e, off1, n1, off2, n2, gamma, checked=False):
    """value [P] with .backward(): the gradient reaches `e` [R, D].  Within one side of one call the problems' row ranges
    must not overlap (ValueError otherwise); side 1 and side 2 may coincide, as in soft_dtw(e, o, n, o, n, gamma).  `e` must
    not be changed in place between the call and its backward (autograd raises if it was).  checked=True: the columns are
    what require_disjoint returned for this call already, and the overlap check is not repeated."""
    if not isinstance(e, torch.Tensor):
        raise ValueError('soft_dtw: e must be a 2-d float32 tensor, not %s' % type(e).__name__)
    return _SoftDtwFunction.apply(e, off1, n1, off2, n2, gamma, bool(checked))
