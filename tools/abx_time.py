"""Times the ABX evaluation (abnet3_amd/abx.py) on a synthetic ZeroSpeech-shaped item set with no audio: 40 phones
with prototype trajectories (4 anchor frames, linearly interpolated) plus noise and a per-speaker offset, items of
3-30 frames, D = 100, 10-20 speakers, 9 contexts; one utterance per speaker with its items end to end, 10 ms frames.

  both modes end to end    ABXEvaluator.run, wall time, and its phases: host enumeration (cells, needed pairs, score
                           rows), distances (abn_dtw_cost_batched + the division), scoring (abn_abx_score)
  abn_dtw_cost_batched     the cost-only kernel alone on the within-speaker mode's pairs (device events)
  abn_dtw_batched          utils.dtw_align_batch on the same pairs (paths + traceback; the same costs, checked bit for bit)
  C oracle                 oracle/dtw_oracle.dtw_batch(..., threads=16) on the same pairs (the same DP on the CPU)

--distance kl times the symmetrised Kullback-Leibler route on the same set pushed through a row softmax (posteriorgrams):

  both modes end to end    ABXEvaluator(distance='kl').run, wall time and phases as above
  abn_kl_tables            the P / L / BAD tables of the whole corpus alone
  abn_dtw_cost_kl_batched  the KL instantiation of the cost kernel alone on the within-speaker mode's pairs
  abn_dtw_cost_batched     the cosine instantiation on the same pair table of the same posteriorgrams, in the same run
  torch                    what a user could write before: the frame-distance matrices alone (no DTW) of the same pairs as
                           a chunked torch expression on the GPU, pairs bucketed by (n1, n2) so that nothing is padded
  --parent-lib FILE        the kernels of another build of the library (the parent commit's) -- abn_dtw_cost_batched, and
                           under --distance kl abn_dtw_cost_kl_batched too -- timed alternately with this build's on the
                           same pairs: several repeats per build, the outputs compared bit for bit.  A route passes when
                           the ratio of the medians is at most 1 + twice the parent's own relative spread over its repeats

Every GPU route settles the clock (untimed calls for 0.3 s) before its timed calls; medians are reported.
python tools/abx_time.py [--items N] [--distance cosine|kl] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
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


def parent_library(path, lib, names):
    """Another build of the library, its entry points `names` typed as this build's are."""
    parent = ctypes.CDLL(os.path.abspath(path))
    for name in names:
        fn, own = getattr(parent, name), getattr(lib, name)
        fn.restype, fn.argtypes = own.restype, own.argtypes
    return parent


def versus_parent(this_fn, parent_fn, outputs, calls=9, repeats=4):
    """The *_vs_parent_build block of one route: median_ms of this build's call and of the parent's, alternating,
    `repeats` times each; outputs() -> [(this build's tensor, the parent's)], compared bit for bit after the last call.
    The bound on the ratio of the medians is 1 + 2 x the parent's relative spread, (max - min) / median, over its repeats."""
    this, other = [], []
    for _ in range(repeats):
        this.append(median_ms(this_fn, calls))
        other.append(median_ms(parent_fn, calls))
    torch.cuda.synchronize()
    ratio = float(np.median(this) / np.median(other))
    spread = float((max(other) - min(other)) / np.median(other))
    same = all(a.dtype == b.dtype and torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in outputs())
    return {'this_build_ms': [round(t, 4) for t in this], 'parent_build_ms': [round(t, 4) for t in other],
            'ratio_of_medians': round(ratio, 4), 'parent_relative_spread': round(spread, 4),
            'bound_on_the_ratio': round(1.0 + 2.0 * spread, 4), 'within_the_bound': bool(ratio <= 1.0 + 2.0 * spread),
            'outputs_bit_identical': bool(same)}


def finish(res, out):
    """Prints and writes the result; a route of *_vs_parent_build whose outputs differ between the builds is an error."""
    print(json.dumps(res))
    if out:
        os.makedirs(os.path.dirname(os.path.abspath(out)), exist_ok=True)
        with open(out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    for key, block in res.items():
        if key.endswith('_vs_parent_build'):
            assert block['outputs_bit_identical'], key


def wall(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return time.perf_counter() - t0, out


def time_modes(ev, calls):
    """({mode: figures}, {mode: plan}) of ABXEvaluator.run and its phases."""
    out, plans = {}, {}
    for mode in ('within', 'across'):
        r = ev.run(mode)                                     # warm
        walls = []
        for _ in range(calls):
            s, r2 = wall(lambda: ev.run(mode))
            walls.append(s)
            assert r2.error == r.error
        t_plan, plan = wall(lambda: ev.plan(mode))
        t_dist, dist = wall(lambda: ev.distances(plan))
        t_score, _ = wall(lambda: abx_score(dist, plan))
        plans[mode] = plan
        out[mode] = {'error_percent': r.error, 'cells': len(r.cells), 'pairs': r.n_pairs, 'triplets': r.n_triplets,
                     'end_to_end_s_median': round(float(np.median(walls)), 4),
                     'phase_s': {'host_enumeration': round(t_plan, 4), 'distances': round(t_dist, 4),
                                 'scoring': round(t_score, 4)}}
    return out, plans


def torch_buckets(off1, n1, off2, n2, chunk=2048):
    """Device row indices ([c, n1], [c, n2]) of the pairs, bucketed by (n1, n2), at most `chunk` pairs each."""
    key = n1.astype(np.int64) * 100000 + n2
    order = np.argsort(key, kind='stable')
    cuts = np.flatnonzero(np.diff(key[order])) + 1
    out = []
    for idx in np.split(order, cuts):
        a, b = int(n1[idx[0]]), int(n2[idx[0]])
        for c0 in range(0, len(idx), chunk):
            sub = idx[c0:c0 + chunk]
            out.append((torch.from_numpy(off1[sub, None] + np.arange(a)[None, :]).cuda(),
                        torch.from_numpy(off2[sub, None] + np.arange(b)[None, :]).cuda()))
    return out


def torch_frame_distances(P, L, buckets):
    """The symmetrised-KL frame-distance matrices of every pair (no DTW), as torch expressions; their sum."""
    total = torch.zeros((), dtype=torch.float64, device=P.device)
    for r1, r2 in buckets:
        d = 0.5 * ((P[r1][:, :, None, :] - P[r2][:, None, :, :]) * (L[r1][:, :, None, :] - L[r2][:, None, :, :])).sum(-1)
        total += d.sum(dtype=torch.float64)
    return total


def main_kl(a):
    items, feats, times, n_spk = synthetic(a.items)
    post = {k: torch.softmax(torch.from_numpy(v), dim=1).numpy() for k, v in feats.items()}
    ev = ABXEvaluator(items, post, times, distance='kl')
    res = {'device': torch.cuda.get_device_name(0),
           'set': '%d items, 40 phones, D = 100, %d speakers, 9 contexts, 3-30 frames per item; row softmax of the '
                  'features' % (len(items), n_spk),
           'distance': 'kl', 'floor': 1e-6}
    res['modes'], plans = time_modes(ev, a.calls)
    wplan = plans['within']
    P, Q = ev.kept[wplan.P], ev.kept[wplan.Q]
    off1, n1, off2, n2 = ev.row[P], ev.n[P], ev.row[Q], ev.n[Q]
    table = ev.corpus.table
    tabs = ev.tables
    lib = _lib.load()
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    d_tab = [dev(off1, np.int64), dev(n1, np.int32), dev(off2, np.int64), dev(n2, np.int32)]
    npairs, rows, D = len(P), table.shape[0], table.shape[1]
    cost = torch.empty(npairs, dtype=torch.float64, device='cuda')
    plen = torch.empty(npairs, dtype=torch.int32, device='cuda')
    ccost, cplen = torch.empty_like(cost), torch.empty_like(plen)

    def kl_kernel(l=lib, c=cost, ln=plen):
        _lib.check(l.abn_dtw_cost_kl_batched(_lib.ptr(tabs.P), _lib.ptr(tabs.L), rows, _lib.ptr(tabs.P), _lib.ptr(tabs.L), rows,
                                             *[_lib.ptr(t) for t in d_tab], npairs, D, _lib.ptr(tabs.bad), _lib.ptr(tabs.bad),
                                             _lib.ptr(c), _lib.ptr(ln), _lib.stream()), 'abn_dtw_cost_kl_batched')

    def cosine_kernel(l=lib, c=ccost, ln=cplen):
        _lib.check(l.abn_dtw_cost_batched(_lib.ptr(table), rows, _lib.ptr(table), rows, *[_lib.ptr(t) for t in d_tab],
                                          npairs, D, _lib.ptr(c), _lib.ptr(ln), _lib.stream()), 'abn_dtw_cost_batched')

    P2, L2, bad2 = torch.empty_like(table), torch.empty_like(table), torch.empty(rows, dtype=torch.uint8, device='cuda')

    def tables_kernel():
        _lib.check(lib.abn_kl_tables(_lib.ptr(table), rows, D, 1e-6, _lib.ptr(P2), _lib.ptr(L2), _lib.ptr(bad2), _lib.stream()),
                   'abn_kl_tables')

    buckets = torch_buckets(off1, n1, off2, n2)
    holder = {}

    def torch_route():
        holder['sum'] = torch_frame_distances(tabs.P, tabs.L, buckets)

    cells = int(np.dot(n1.astype(np.int64), n2.astype(np.int64)))
    kl_ms = median_ms(kl_kernel)
    cos_ms = median_ms(cosine_kernel)
    tab_ms = median_ms(tables_kernel)
    torch_ms = median_ms(torch_route, calls=3)
    kl_ms2 = median_ms(kl_kernel)
    rate = lambda ms: {'pairs_per_s': round(npairs / (ms * 1e-3), 1), 'cells_per_s': round(cells / (ms * 1e-3), 1)}
    res['kernels_on_within_pairs'] = {
        'pairs': npairs, 'cells': cells, 'mean_cells_per_pair': round(cells / max(npairs, 1), 2), 'table_rows': rows,
        'abn_dtw_cost_kl_batched_ms': round(kl_ms, 4), 'abn_dtw_cost_kl_batched_ms_again': round(kl_ms2, 4),
        'abn_dtw_cost_batched_ms_same_pairs': round(cos_ms, 4), 'kl_over_cosine': round(kl_ms / cos_ms, 3),
        'abn_kl_tables_ms': round(tab_ms, 4),
        'torch_frame_distances_ms': round(torch_ms, 3),
        'torch_frame_distances_is': 'frame-distance matrices alone (no DTW), %d bucketed torch expressions' % len(buckets),
        'torch_over_kl_kernel': round(torch_ms / kl_ms, 2),
        'kl_kernel': rate(kl_ms), 'cosine_kernel': rate(cos_ms),
        'pairs_dropped': int((plen <= 0).sum().item())}
    if a.parent_lib:
        parent = parent_library(a.parent_lib, lib, ['abn_dtw_cost_batched', 'abn_dtw_cost_kl_batched'])
        pcost, pplen = torch.empty_like(cost), torch.empty_like(plen)
        res['cosine_kernel_vs_parent_build'] = versus_parent(cosine_kernel, lambda: cosine_kernel(parent, pcost, pplen),
                                                             lambda: [(ccost, pcost), (cplen, pplen)])
        res['kl_kernel_vs_parent_build'] = versus_parent(kl_kernel, lambda: kl_kernel(parent, pcost, pplen),
                                                         lambda: [(cost, pcost), (plen, pplen)])
    finish(res, a.out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--items', type=int, default=6000)
    ap.add_argument('--calls', type=int, default=3)
    ap.add_argument('--distance', choices=('cosine', 'kl'), default='cosine')
    ap.add_argument('--parent-lib', default=None, help="another build of the library (the parent commit's) to time the cost kernels of")
    ap.add_argument('--out', default=None, help='default: profiles/abx_time.json, profiles/abx_kl_time.json under --distance kl')
    a = ap.parse_args()
    if a.out is None:
        a.out = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'profiles',
                             'abx_kl_time.json' if a.distance == 'kl' else 'abx_time.json')
    if a.distance == 'kl':
        return main_kl(a)
    items, feats, times, n_spk = synthetic(a.items)
    ev = ABXEvaluator(items, feats, times)
    res = {'device': torch.cuda.get_device_name(0),
           'set': '%d items, 40 phones, D = 100, %d speakers, 9 contexts, 3-30 frames per item' % (len(items), n_spk)}
    res['modes'], plans = time_modes(ev, a.calls)
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

    def cost_kernel(l=lib, c=cost, ln=plen):
        _lib.check(l.abn_dtw_cost_batched(_lib.ptr(table), table.shape[0], _lib.ptr(table), table.shape[0],
                                          *[_lib.ptr(t) for t in d_tab], npairs, table.shape[1], _lib.ptr(c),
                                          _lib.ptr(ln), _lib.stream()), 'abn_dtw_cost_batched')

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
    if a.parent_lib:
        parent = parent_library(a.parent_lib, lib, ['abn_dtw_cost_batched'])
        pcost, pplen = torch.empty_like(cost), torch.empty_like(plen)
        res['cost_kernel_vs_parent_build'] = versus_parent(cost_kernel, lambda: cost_kernel(parent, pcost, pplen),
                                                           lambda: [(cost, pcost), (plen, pplen)])
    finish(res, a.out)


if __name__ == '__main__':
    main()
