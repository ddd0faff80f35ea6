"""A synthetic batch plan and its oracle pass (test infrastructure: numpy only, torch where a plan is uploaded).

What TrainerSiamese._run_planned trains on is a abnet3_amd.dataloader.BatchPlan: one table of frames, two index lists,
the labels, and per batch an (offset, size) span.  host_plan() draws such a plan with numpy -- batches of chosen sizes,
STORED in another order than they are visited, rows repeated between and inside batches -- upload() puts it on the device,
PlanLoader is the loader surface _planned() asks for, and oracle_pass() is the pass the reference's loop would run on it:
every batch gathered on the host with plain numpy indexing and stepped by oracle.siamese_np.train_step.
"""
import numpy as np

from oracle import siamese_np as O


def host_plan(rng, D, sizes, label_dtype=np.float64, table_rows=None, scatter=True, has_arrays=None):
    """The host arrays of a plan whose k-th visited batch has sizes[k] frame pairs.

    scatter: the batches lie in the index lists in a random order (order[k] = the id of the k-th visited batch), so that
    a step's offset is not the sum of the sizes visited before it.  Rows behind table_rows never occur; every row of a
    table smaller than the pair count occurs more than once."""
    sizes = [int(s) for s in sizes]
    total = sum(sizes)
    if table_rows is None:
        table_rows = max(8, total // 3)
    order = rng.permutation(len(sizes)) if scatter else np.arange(len(sizes))      # step k visits batch order[k]
    stored = np.zeros(len(sizes), dtype=np.int64)
    stored[order] = sizes                                                          # size of batch id b
    offsets = np.concatenate([[0], np.cumsum(stored)]).astype(np.int64)
    # (a frame is never paired with itself: such a pair's cosine is exactly 1 and a lone 'same' pair's loss exactly 0, which
    # no relative bar can hold a kernel to)
    idx1 = rng.integers(0, table_rows, total).astype(np.int64)
    return dict(table=rng.standard_normal((table_rows, D)).astype(np.float32),
                idx1=idx1, idx2=((idx1 + rng.integers(1, table_rows, total)) % table_rows).astype(np.int64),
                labels=rng.choice([1, -1], total).astype(label_dtype),
                offsets=offsets, order=[int(b) for b in order],
                has_arrays=None if has_arrays is None else np.asarray(has_arrays, dtype=bool)[np.argsort(order)])


def upload(host, order=None):
    """The BatchPlan of host_plan()'s arrays on the current device (fresh device arrays on every call)."""
    import torch
    from abnet3_amd.dataloader import BatchPlan
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return BatchPlan(dev(host['table']), dev(host['idx1']), dev(host['idx2']), dev(host['labels']), host['offsets'],
                     host['order'] if order is None else order, has_arrays=host['has_arrays'])


def make_plan(rng, D, sizes, label_dtype=np.float64, table_rows=None, **kw):
    """(BatchPlan on the device, its host arrays)."""
    host = host_plan(rng, D, sizes, label_dtype, table_rows, **kw)
    return upload(host), host


class PlanLoader(object):
    """The loader surface of a planned pass: plan(train_mode), and batch_iterator(train_mode) = the plan's batches one by
    one (what TrainerSiamese takes with planned_passes = False)."""

    def __init__(self, train_plan, dev_plan=None):
        self.plans = {True: train_plan, False: dev_plan if dev_plan is not None else train_plan}

    def plan(self, train_mode):
        return self.plans[bool(train_mode)]

    def batch_iterator(self, train_mode):
        return iter(self.plans[bool(train_mode)])

    def whoami(self):
        return {'params': None, 'class_name': type(self).__name__}


def gather_batch(host, b):
    """Batch b as the reference's iterator would yield it: (X1, X2, y); an index outside the table reads a zero row
    (abn_gather_pairs' rule)."""
    first, last = int(host['offsets'][b]), int(host['offsets'][b + 1])
    table = host['table']

    def rows(idx):
        idx = idx[first:last]
        inside = (idx >= 0) & (idx < table.shape[0])
        out = np.zeros((len(idx), table.shape[1]), dtype=np.float32)
        out[inside] = table[idx[inside]]
        return out
    return rows(host['idx1']), rows(host['idx2']), host['labels'][first:last]


def oracle_pass(params, host, spec, opt, loss_kind='coscos2', margin=0.5, avg=False, order=None):
    """One pass of the reference's loop over the plan: ([loss of step k], parameters afterwards).  `params` is stepped
    in place (a dict of float32 arrays keyed like state_dict()); opt = an oracle.siamese_np.Optimizer, or None for a
    pass that only evaluates the training-mode loss of every batch.  A batch of zero frames (the reference's iterator
    yields it): a sum over no pairs is 0, a mean 0 / 0, every gradient is a sum over no rows and the optimizer steps on
    those zeros (torch: momentum and running averages move on); without BatchNorm, whose forward raises on no rows."""
    losses = []
    for b in (host['order'] if order is None else order):
        x1, x2, y = gather_batch(host, b)
        if len(y) == 0:
            assert not spec.batch_norm
            losses.append(float('nan') if avg else 0.0)
            if opt is not None:
                opt.step(params, {k: np.zeros_like(params[k]) for k in spec.param_keys()}, spec.param_keys())
            continue
        loss, _, _ = O.train_step(params, x1, x2, y, spec, opt, loss_kind, margin, avg, do_training=opt is not None)
        losses.append(float(loss))
    return np.array(losses), params
