"""Times the ABX evaluation (abnet3_amd/abx.py) on a synthetic ZeroSpeech-shaped item set with no audio: 40 phones
with prototype trajectories (4 anchor frames, linearly interpolated) plus noise and a per-speaker offset, items of
3-30 frames, D = 100, 10-20 speakers, 9 contexts; one utterance per speaker with its items end to end, 10 ms frames.

  both modes end to end    ABXEvaluator.run, wall time, and its phases: host enumeration (cells, needed pairs, score
                           rows), distances (abn_dtw_cost_batched + the division), scoring (abn_abx_score)
  abn_dtw_cost_batched     the cost-only kernel alone on the within-speaker mode's pairs (device events)
  abn_dtw_batched          utils.dtw_align_batch on the same pairs (paths + traceback; the same costs, checked bit for bit)
  C oracle                 oracle/dtw_oracle.dtw_batch(..., threads=16) on the same pairs (the same DP on the CPU)

Every GPU route settles the clock (untimed calls for 0.3 s) before its timed calls; medians are reported.
python tools/abx_time.py [--items N] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from abnet3_amd import _lib
from abnet3_amd.abx import ABXEvaluator, Items, abx_score, dtw_cost_batch
from abnet3_amd.utils import dtw_align_batch


def synthetic(n_items, D=100, n_phones=40, seed=0):
    rng = np.random.default_rng(seed)
    protos = rng.standard_normal((n_phones, 4, D)).astype(np.float32)
    n_spk = int(rng.integers(10, 21))
    spk_off = 0.3 * rng.standard_normal((n_spk, D)).astype(np.float32)
    phone = rng.integers(0, n_phones, n_items)
    ctx = rng.integers(0, 3, (n_items, 2))
    spk = rng.integers(0, n_spk, n_items)
    cols, feats, times = [], {}, {}
    for s in range(n_spk):
        name, rows, t = 'spk%02d' % s, [], 0
        for i in np.flatnonzero(spk == s):
            n = int(rng.integers(3, 31))
            src = np.linspace(0, 3, n)
            lo = np.minimum(np.floor(src).astype(int), 2)
            w = (src - lo)[:, None].astype(np.float32)
            f = protos[phone[i], lo] * (1 - w) + protos[phone[i], lo + 1] * w + spk_off[s]
            rows.append(f + 1.5 * rng.standard_normal((n, D)).astype(np.float32))
            cols.append((name, (t + 0.5) * 0.01, (t + n - 0.5) * 0.01, 'ph%02d' % phone[i], 'c%d' % ctx[i, 0],
                         'c%d' % ctx[i, 1], name))
            t += n
        if rows:
            feats[name] = np.concatenate(rows).astype(np.float32)
            times[name] = (np.arange(t) + 0.5) * 0.01
    return Items(*zip(*cols)), feats, times, n_spk


def settle(fn, seconds=0.3):
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def median_ms(fn, calls=9):
    settle(fn)
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return float(np.median(ts))


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=6000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))),
                                                  'profiles', 'abx_time.json'))
    a = ap.parse_args()
    items, feats, times, n_spk = synthetic(a.items)
    ev = ABXEvaluator(items, feats, times)
    res = {'device': torch.cuda.get_device_name(0),
           'set': '%d items, 40 phones, D = 100, %d speakers, 9 contexts, 3-30 frames per item' % (len(items), n_spk),
           'modes': {}}
    plans = {}
    for mode in ('within', 'across'):
        r = ev.run(mode)                                     # warm
        walls = []
        for _ in range(a.calls):
            s, r2 = wall(lambda: ev.run(mode))
            walls.append(s)
            assert r2.error == r.error
        t_plan, plan = wall(lambda: ev.plan(mode))
        t_dist, dist = wall(lambda: ev.distances(plan))
        t_score, _ = wall(lambda: abx_score(dist, plan))
        plans[mode] = plan
        res['modes'][mode] = {'error_percent': r.error, 'cells': len(r.cells), 'pairs': r.n_pairs, 'triplets': r.n_triplets,
                              'end_to_end_s_median': round(float(np.median(walls)), 4),
                              'phase_s': {'host_enumeration': round(t_plan, 4), 'distances': round(t_dist, 4),
                                          'scoring': round(t_score, 4)}}
    # the kernels alone, on the within-speaker pairs
    wplan = plans['within']
    P, Q = ev.kept[wplan.P], ev.kept[wplan.Q]
    off1, n1, off2, n2 = ev.row[P], ev.n[P], ev.row[Q], ev.n[Q]
    table = ev.corpus.table
    lib = _lib.load()
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    d_tab = [dev(off1, np.int64), dev(n1, np.int32), dev(off2, np.int64), dev(n2, np.int32)]
    npairs = len(P)
    cost = torch.empty(npairs, dtype=torch.float64, device='cuda')
    plen = torch.empty(npairs, dtype=torch.int32, device='cuda')

    def cost_kernel():
        _lib.check(lib.abn_dtw_cost_batched(_lib.ptr(table), table.shape[0], _lib.ptr(table), table.shape[0],
                                            *[_lib.ptr(t) for t in d_tab], npairs, table.shape[1], _lib.ptr(cost),
                                            _lib.ptr(plen), _lib.stream()), 'abn_dtw_cost_batched')

    holder = {}

    def full_dtw():
        holder['r'] = dtw_align_batch(table, off1, n1, table, off2, n2)

    cells = int(np.dot(n1.astype(np.int64), n2.astype(np.int64)))
    k_ms = median_ms(cost_kernel)
    b_ms = median_ms(full_dtw)
    c, ln = dtw_cost_batch(table, off1, n1, table, off2, n2)
    same = (np.array_equal(c.cpu().numpy().view(np.int64), holder['r'].total_cost.cpu().numpy().view(np.int64)) and
            np.array_equal(ln.cpu().numpy(), holder['r'].path_len.cpu().numpy()))
    from oracle import dtw_oracle as O
    f = table.cpu().numpy()
    stride = int((n1 + n2).max())
    O.dtw_batch(f, off1[:100], n1[:100], f, off2[:100], n2[:100], stride, threads=16)      # warm (OpenMP pool)
    t0 = time.perf_counter()
    O.dtw_batch(f, off1, n1, f, off2, n2, stride, threads=16)
    o_s = time.perf_counter() - t0
    rate = lambda s: {'pairs_per_s': round(npairs / s, 1), 'cells_per_s': round(cells / s, 1)}
    res['kernels_on_within_pairs'] = {
        'pairs': npairs, 'cells': cells, 'mean_cells_per_pair': round(cells / max(npairs, 1), 2),
        'abn_dtw_cost_batched_ms': round(k_ms, 4), 'abn_dtw_batched_ms': round(b_ms, 4),
        'abn_dtw_batched_ms_is': 'one utils.dtw_align_batch call: host staging + fill + traceback',
        'oracle_16_threads_ms': round(o_s * 1e3, 2),
        'cost_kernel': rate(k_ms * 1e-3), 'dtw_batched': rate(b_ms * 1e-3), 'oracle_16_threads': rate(o_s),
        'cost_kernel_speedup_over_dtw_batched': round(b_ms / k_ms, 3),
        'cost_kernel_speedup_over_oracle_16_threads': round(o_s * 1e3 / k_ms, 2),
        'costs_and_lengths_bit_identical': bool(same)}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
