"""tests/plan_np.py itself (no GPU): the synthetic plan is laid out as a BatchPlan reads it and the oracle pass is the
reference's loop over its batches."""
import numpy as np

import plan_np
from oracle import siamese_np as O


def _params(rng, spec):
    p = {}
    for l in range(spec.n_layers):
        p[spec.lin_keys[l] + '.weight'] = (rng.standard_normal((spec.dims[l + 1], spec.dims[l])) / np.sqrt(spec.dims[l])).astype(np.float32)
        p[spec.lin_keys[l] + '.bias'] = (0.1 * rng.standard_normal(spec.dims[l + 1])).astype(np.float32)
    return p


def test_a_scattered_plan_visits_the_requested_sizes():
    sizes = [1, 31, 0, 33, 64, 2]
    host = plan_np.host_plan(np.random.default_rng(0), 12, sizes, np.int8, has_arrays=[True] * 6)
    spans = [(host['offsets'][b], host['offsets'][b + 1] - host['offsets'][b]) for b in host['order']]
    assert [int(n) for _, n in spans] == sizes
    assert sorted(host['order']) == list(range(6)) and host['order'] != list(range(6))
    assert [int(f) for f, _ in spans] != list(np.cumsum([0] + sizes[:-1]))          # offsets are not the visited sizes' running sum
    assert host['labels'].dtype == np.int8 and set(np.unique(host['labels'])) == {-1, 1}
    assert host['idx1'].dtype == np.int64 and host['idx1'].max() < host['table'].shape[0]
    assert len(np.unique(host['idx1'])) < len(host['idx1'])                           # repeated rows
    x1, x2, y = plan_np.gather_batch(host, host['order'][3])
    first = int(host['offsets'][host['order'][3]])
    assert x1.shape == (33, 12) and np.array_equal(x2[5], host['table'][host['idx2'][first + 5]]) and len(y) == 33


def test_rows_outside_the_table_read_as_zeros():
    host = plan_np.host_plan(np.random.default_rng(1), 8, [4], scatter=False)
    host['idx1'][1], host['idx2'][2] = -1, host['table'].shape[0]
    x1, x2, _ = plan_np.gather_batch(host, 0)
    assert not x1[1].any() and not x2[2].any() and x1[0].any() and x2[1].any()


def test_the_oracle_pass_is_the_loop_over_the_batches():
    rng = np.random.default_rng(2)
    spec = O.TowerSpec(12, 1, 16, 8, 'sigmoid')
    host = plan_np.host_plan(rng, 12, [5, 0, 33, 7])
    p0 = _params(rng, spec)
    losses, after = plan_np.oracle_pass({k: v.copy() for k, v in p0.items()}, host, spec, O.Optimizer('adadelta', 0.1), 'cosmargin', 0.3, True)
    p, opt, want = {k: v.copy() for k, v in p0.items()}, O.Optimizer('adadelta', 0.1), []
    for b in host['order']:
        sl = slice(host['offsets'][b], host['offsets'][b + 1])
        if sl.stop > sl.start:
            want.append(O.train_step(p, host['table'][host['idx1'][sl]], host['table'][host['idx2'][sl]], host['labels'][sl], spec, opt,
                                     'cosmargin', 0.3, True)[0])
        else:                                      # the empty batch: a step on zero gradients (Adadelta's averages decay)
            opt.step(p, {k: np.zeros_like(v) for k, v in p.items()}, spec.param_keys())
    assert np.isnan(losses[1]) and np.array_equal(np.delete(losses, 1), want)          # (a mean over no pairs)
    assert all(np.array_equal(after[k], p[k]) for k in p) and any(not np.array_equal(after[k], p0[k]) for k in p)
    frozen, same = plan_np.oracle_pass({k: v.copy() for k, v in p0.items()}, host, spec, None)
    assert all(np.array_equal(same[k], p0[k]) for k in p0) and frozen[1] == 0.0 and (np.delete(frozen, 1) > 0).all()
