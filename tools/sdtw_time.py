"""Times abnq_softdtw_forward / abnq_softdtw_backward (abnet3_amd/csrc/softdtw.hip, abnet3_amd/softdtw.py) and one
TrainerSequencePairs step, and records the kernels' accuracy against tests/sdtw_np.py.

Workloads: P = 16, 64, 256, 4096 word pairs, lengths drawn from 20 .. 120 on either side, D = 100.  Per workload, each the
median of 15 calls between device events after 0.3 s of untimed calls (tools/gmm_time.py's median_ms); a soft-DTW call reads
its problem table back and waits for the stream, so a call's time is its latency, enqueue included:

  forward           soft_dtw_batch(keep=True): norms, cells, sweep, r stored
  forward value     soft_dtw_batch(keep=False): the same without r (the dev pass)
  backward          soft_dtw_backward on the forward's handle: the E sweep and both gradient blocks
  dtw cost          abx.dtw_cost_batch (abn_dtw_cost_batched) on the same pair table, for orientation: the nearest existing
                    kernel, a wavefront per pair, angular cells, no transcendental work in its sweep.  Context, not a bar.

`what_limits` separates the phases by measurement: ONE problem of 120 x 120 at D = 100 and at D = 4 (the cell phase and the
gradient sums shrink 25-fold, the sweeps do not), and 120 x 120 against 30 x 30 at D = 4 (the sweeps shrink 4-fold in steps,
16-fold in cells); the time per anti-diagonal step of a sweep follows from the small-D figures.  `grid` times P = 4096 under
ABN_SDTW_GRID = 256, 512, 1024 and the default 2048: one, two and four workgroups resident per CU (the kernels' registers
allow four), and four resident with four more queued.

`step`: a SiameseNetwork 280 -> 500 x 2 -> 100 (sigmoid) on 64 word pairs of 20 .. 120 frames through
TrainerSequencePairs.train_step (SGD), with the loss's share (SoftDTWLoss.value_and_grad on the embeddings) beside it.

`accuracy`: for every case of tests/test_gpu_sdtw.py the value's error against its derived bar and the ratio of the kernel's
gradient error to the float32-cell yardstick's, both against the float64 restatement.  No threshold is set here.

python tools/sdtw_time.py [--out FILE] [--skip-accuracy]"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tests'))
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np

from gmm_time import median_ms


def pair_table(P, lo, hi, D, seed=0):
    """(e [rows, D] on the device, off1, n1, off2, n2 on the host): every pair's two tokens end to end."""
    import torch
    rng = np.random.default_rng(seed)
    n1, n2 = rng.integers(lo, hi + 1, P).astype(np.int32), rng.integers(lo, hi + 1, P).astype(np.int32)
    off1 = (np.cumsum(n1 + n2) - n1 - n2).astype(np.int64)
    off2 = off1 + n1
    e = torch.from_numpy(rng.standard_normal((int((n1 + n2).sum()), D)).astype(np.float32)).cuda()
    return e, off1, n1, off2, n2


def time_table(e, off1, n1, off2, n2, gamma=0.1, with_dtw=True):
    import torch
    from abnet3_amd import abx, softdtw
    P = len(n1)
    cells = int((n1.astype(np.int64) * n2).sum())
    hold = {}
    w = torch.ones(P, device='cuda')

    def fwd():
        hold['f'] = softdtw.soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=True)

    def fwd_value():
        hold['v'] = softdtw.soft_dtw_batch(e, off1, n1, off2, n2, gamma, keep=False)

    def bwd():
        hold['b'] = softdtw.soft_dtw_backward(hold['f'][1], w)

    def dtw():
        hold['d'] = abx.dtw_cost_batch(e, off1, n1, e, off2, n2)

    res = {'P': P, 'D': int(e.shape[1]), 'cells': cells, 'steps_longest': int((n1 + n2 - 1).max()),
           'forward': median_ms(fwd), 'forward_value': median_ms(fwd_value)}
    fwd()
    res['backward'] = median_ms(bwd)
    if with_dtw:
        res['dtw_cost'] = median_ms(dtw)
    res['forward_again'] = median_ms(fwd)
    for k in ('forward', 'forward_value', 'backward') + (('dtw_cost',) if with_dtw else ()):
        res[k]['cells_per_s'] = round(cells / (res[k]['median_ms'] * 1e-3), 1)
    res['workspace_bytes'] = int(hold['f'][1].ws.numel())
    return res


def one_problem(n, D, gamma=0.1):
    e, off1, n1, off2, n2 = pair_table(1, n, n, D, seed=n + D)
    r = time_table(e, off1, n1, off2, n2, gamma, with_dtw=False)
    return {'n': n, 'm': n, 'D': D, 'forward_ms': r['forward']['median_ms'], 'forward_value_ms': r['forward_value']['median_ms'],
            'backward_ms': r['backward']['median_ms'], 'steps': 2 * n - 1}


def what_limits():
    a, b, c = one_problem(120, 100), one_problem(120, 4), one_problem(30, 4)
    out = {'one_problem': [a, b, c]}
    # two sizes at D = 4: time = fixed + steps * per_step (the cell phase at D = 4 is a few hundred fmaf per thread)
    for key in ('forward_ms', 'backward_ms'):
        per_step_us = (b[key] - c[key]) * 1e3 / (b['steps'] - c['steps'])
        out[key.replace('_ms', '')] = {
            'us_per_antidiagonal_step': round(per_step_us, 4),
            'fixed_us': round(c[key] * 1e3 - per_step_us * c['steps'], 2),
            'sweep_share_at_120x120_D100': round(per_step_us * a['steps'] / (a[key] * 1e3), 3),
            'ms_added_by_D_4_to_100_at_120x120': round(a[key] - b[key], 4)}
    return out


def grid_effect():
    e, off1, n1, off2, n2 = pair_table(4096, 20, 120, 100)
    out = {}
    for grid in ('256', '512', '1024', '2048'):
        os.environ['ABN_SDTW_GRID'] = grid
        r = time_table(e, off1, n1, off2, n2, with_dtw=False)
        out['grid_' + grid] = {'forward_ms': r['forward']['median_ms'], 'backward_ms': r['backward']['median_ms']}
    del os.environ['ABN_SDTW_GRID']
    return out


def step_workload(P=64):
    import torch
    from abnet3_amd.loss import SoftDTWLoss
    from abnet3_amd.model import SiameseNetwork
    from abnet3_amd.trainer import TrainerSequencePairs
    torch.manual_seed(0)
    net = SiameseNetwork(input_dim=280, num_hidden_layers=1, hidden_dim=500, output_dim=100, activation_layer='sigmoid', p_dropout=0.0,
                         batch_norm=False, output_path='/tmp/abn_sdtw_time')
    f = SoftDTWLoss()
    tr = TrainerSequencePairs(network=net, loss=f, optimizer_type='sgd', lr=0.01, dataloader=None, log_dir='/tmp/abn_sdtw_time_runs')
    net.train()
    X, off1, n1, off2, n2 = pair_table(P, 20, 120, 280, seed=3)
    # side 1's tokens first, then side 2's, as the loader lays a batch out: the offsets above interleave, which is as valid
    y = torch.from_numpy(np.where(np.arange(P) % 2, 1, -1).astype(np.int64)).cuda()
    batch = (X, off1, n1, off2, n2, y)
    hold = {}

    def step():
        hold['s'] = tr.train_step(batch, True)

    with torch.no_grad():
        emb = net.forward_once(X)

    def loss_only():
        hold['l'] = f.value_and_grad(emb, off1, n1, off2, n2, y)

    res = {'pairs': P, 'rows': int(X.shape[0]), 'network': '280 -> 500 x 2 -> 100, sigmoid', 'optimizer': 'sgd',
           'first_loss': float(tr.train_step(batch, False)), 'trainer_step': median_ms(step), 'loss_value_and_grad': median_ms(loss_only)}
    res['trainer_step_again'] = median_ms(step)
    res['last_loss'] = float(tr.train_step(batch, False))
    return res


def accuracy():
    import test_gpu_sdtw as T
    import torch
    rows, worst, worst_value = [], 0.0, 0.0
    for n, m, D, gamma in T.CASES:
        c = T.case(n, m, D, gamma)
        e = torch.from_numpy(np.concatenate([c['x'], c['y']])).cuda()
        value, g1, g2 = T.run(e, [0], [n], [n], [m], gamma)
        ref, yard = c['ref'], c['yard']
        yerr = float(max(np.abs(yard['g1'] - ref['g1']).max(), np.abs(yard['g2'] - ref['g2']).max()))
        gerr = float(max(np.abs(g1 - ref['g1']).max(), np.abs(g2 - ref['g2']).max()))
        verr, vbar = abs(float(value[0]) - ref['value']), T.value_bar(n, m, D, ref['value'])
        ratio = gerr / yerr if yerr > 0 else (0.0 if gerr == 0 else float('inf'))
        rows.append({'n': n, 'm': m, 'D': D, 'gamma': gamma, 'value_error': verr, 'value_bar': vbar, 'value_error_over_bar': verr / vbar,
                     'yardstick_value_error': abs(yard['value'] - ref['value']), 'gradient_error': gerr,
                     'yardstick_gradient_error': yerr, 'kernel_over_yardstick': ratio,
                     'max_abs_gradient': float(max(np.abs(ref['g1']).max(), np.abs(ref['g2']).max()))})
        worst, worst_value = max(worst, ratio), max(worst_value, verr / vbar)
    return {'cases': rows, 'worst_kernel_over_yardstick': worst, 'worst_value_error_over_bar': worst_value, 'factor_allowed': 16}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sdtw_time.json'))
    ap.add_argument('--skip-accuracy', action='store_true')
    a = ap.parse_args()
    import torch
    from abnet3_amd import softdtw
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'gamma': 0.1, 'lengths': [20, 120],
           'max_len': softdtw.max_len(), 'max_d': softdtw.max_d(),
           'workloads': [time_table(*pair_table(P, 20, 120, 100)) for P in (16, 64, 256, 4096)],
           'what_limits': what_limits(), 'grid': grid_effect(), 'step': step_workload()}
    if not a.skip_accuracy:
        res['accuracy'] = accuracy()
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
