"""Times the batched edit-distance kernel (abnet3_amd/csrc/edit.hip) and TermEvaluator (abnet3_amd/tde.py).

Shapes:
  ned    2,000,000 pairs, lengths 3-30, alphabet 40: the within-cluster pairs of a few thousand discovered clusters
  units  150,607 pairs (the ABX bench's within-speaker pair count), lengths 3-30, alphabet 1024: unit-id sequences

Timed, per shape (device events; every route settles the clock with untimed calls for 0.3 s before its 15 timed calls;
medians, minima and maxima are reported):

  kernel            abn_edit_distance_batched on the table sorted by (short, long) as edit_distance_batch sorts it, with
                    max_short = 32, 64 and 256: the three instantiations on the same pairs -- and on the unsorted table
  wrapper           edit_distance_batch: sort, launch, un-sort
  torch route       the only way to do it before this kernel, same GPU, same process, alternating: a batched row DP over
                    the padded [P, longest] table, one step per row of the other side, the left dependence resolved by a
                    cummin of row - j; checked once against the kernel for equality
  numpy             tests/tde_np.py's plain DP on a sample of the pairs, for scale (pairs/s on one CPU core)

DP cells = the sum of n1 x n2 over the pairs.  Then TermEvaluator.evaluate end to end on a synthetic alignment (wall
clock), split into transcription, pair table, kernel (upload, sort, launch, download) and reduction.

python tools/tde_time.py [--pairs 2000000] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), 'tests'))
import numpy as np

from gmm_time import median_ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_route(A, B, n1, n2):
    """Levenshtein distances [P] of the padded int32 tables A [P, L1] and B [P, L2] with lengths n1, n2."""
    import torch
    P, L2 = B.shape
    ramp = torch.arange(L2 + 1, device=A.device, dtype=torch.int32)
    row = ramp.repeat(P, 1)
    at = n2.to(torch.int64)[:, None]
    res = torch.where(n1 == 0, n2, torch.zeros_like(n2))
    for i in range(A.shape[1]):
        cur = torch.empty_like(row)
        cur[:, 0] = i + 1
        cur[:, 1:] = torch.minimum(row[:, 1:] + 1, row[:, :-1] + (B != A[:, i:i + 1]).to(torch.int32))
        row = torch.cummin(cur - ramp, dim=1).values + ramp
        res = torch.where(n1 == i + 1, row.gather(1, at)[:, 0], res)
    return res


def raw(lib, _lib, t, cols, P, max_short, out):
    _lib.check(lib.abn_edit_distance_batched(_lib.ptr(t), t.numel(), _lib.ptr(t), t.numel(), *[_lib.ptr(c) for c in cols], P,
                                             max_short, _lib.ptr(out), _lib.stream()), 'abn_edit_distance_batched')


def shape(name, P, alphabet, seed, numpy_sample=2000):
    import torch
    import tde_np
    from abnet3_amd import _lib, tde
    lib = _lib.load()
    rng = np.random.default_rng(seed)
    n1, n2 = rng.integers(3, 31, P).astype(np.int32), rng.integers(3, 31, P).astype(np.int32)
    o1 = np.cumsum(n1, dtype=np.int64) - n1
    o2 = int(n1.sum()) + np.cumsum(n2, dtype=np.int64) - n2
    table = rng.integers(0, alphabet, int(n1.sum()) + int(n2.sum())).astype(np.int32)
    cells = float((n1.astype(np.int64) * n2).sum())
    res = {'shape': name, 'pairs': P, 'alphabet': alphabet, 'lengths': '3-30', 'dp_cells': cells}
    t = torch.from_numpy(table).cuda()
    d = [torch.from_numpy(a).cuda() for a in (o1, n1, o2, n2)]
    order = torch.argsort((torch.minimum(d[1], d[3]).to(torch.int64) << 32) + torch.maximum(d[1], d[3]).to(torch.int64))
    srt = [c[order].contiguous() for c in d]
    out = torch.empty(P, dtype=torch.int32, device='cuda')
    hold = {}

    def rate(r):
        s = r['median_ms'] * 1e-3
        return dict(r, pairs_per_s=round(P / s), dp_cells_per_s=round(cells / s))

    # the padded tables of the torch route (built once, untimed)
    L = 30
    idx = torch.arange(L, device='cuda')[None, :]
    A = torch.where(idx < d[1][:, None], t[(d[0][:, None] + idx).clamp_(max=t.numel() - 1)], torch.full((1, 1), -1, dtype=torch.int32, device='cuda'))
    B = torch.where(idx < d[3][:, None], t[(d[2][:, None] + idx).clamp_(max=t.numel() - 1)], torch.full((1, 1), -2, dtype=torch.int32, device='cuda'))

    def t_route():
        hold['t'] = torch_route(A, B, d[1], d[3])

    # alternating: kernel, torch, kernel, ...
    res['kernel_sorted_max_short_32'] = rate(median_ms(lambda: raw(lib, _lib, t, srt, P, 32, out)))
    res['torch_route'] = rate(median_ms(t_route))
    res['kernel_sorted_max_short_64'] = rate(median_ms(lambda: raw(lib, _lib, t, srt, P, 64, out)))
    res['kernel_sorted_max_short_256'] = rate(median_ms(lambda: raw(lib, _lib, t, srt, P, 256, out)))
    res['kernel_unsorted_max_short_32'] = rate(median_ms(lambda: raw(lib, _lib, t, d, P, 32, out)))
    res['kernel_sorted_max_short_32_again'] = rate(median_ms(lambda: raw(lib, _lib, t, srt, P, 32, out)))
    res['wrapper_edit_distance_batch'] = rate(median_ms(lambda: hold.__setitem__('w', tde.edit_distance_batch(t, d[0], d[1], t, d[2], d[3], max_short=32))))
    res['speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / res['kernel_sorted_max_short_32']['median_ms'], 2)
    res['wrapper_speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / res['wrapper_edit_distance_batch']['median_ms'], 2)
    raw(lib, _lib, t, d, P, 32, out)
    torch.cuda.synchronize()
    res['torch_route_equals_kernel'] = bool(torch.equal(hold['t'], out)) and bool(torch.equal(hold['w'], out))
    got = out[:numpy_sample].cpu().numpy()
    t0 = time.perf_counter()
    ref = tde_np.edit_batch(table, o1[:numpy_sample], n1[:numpy_sample], table, o2[:numpy_sample], n2[:numpy_sample], 32)
    dt = time.perf_counter() - t0
    res['numpy_restatement'] = {'sample_pairs': numpy_sample, 'pairs_per_s': round(numpy_sample / dt), 'equals_kernel': bool(np.array_equal(ref, got))}
    del A, B, hold
    torch.cuda.empty_cache()
    return res


def end_to_end(n_files=400, n_clusters=3000, seed=5):
    """TermEvaluator.evaluate on a synthetic alignment: files of 1500-2500 phones of 30-150 ms over 40 symbols, clusters
    of 10-40 tokens of 0.2-1.5 s."""
    import torch
    from abnet3_amd import tde
    rng = np.random.default_rng(seed)
    files, on, off, sym, ends = [], [], [], [], []
    for f in range(n_files):
        d = rng.uniform(0.03, 0.15, int(rng.integers(1500, 2501)))
        e = np.cumsum(d)
        files += ['f%04d' % f] * len(d)
        on.append(e - d), off.append(e), sym.append(rng.integers(0, 40, len(d))), ends.append(e[-1])
    symbols = np.array(['SIL'] + ['p%02d' % k for k in range(39)])
    a = tde.make_alignment(files, np.concatenate(on), np.concatenate(off), symbols[np.concatenate(sym)])
    clusters = []
    for _ in range(n_clusters):
        c = []
        for _ in range(int(rng.integers(10, 41))):
            f = int(rng.integers(0, n_files))
            t0 = float(rng.uniform(0, ends[f] - 2.0))
            c.append(('f%04d' % f, t0, t0 + float(rng.uniform(0.2, 1.5))))
        clusters.append(c)
    ev = tde.TermEvaluator(a, ignore=('SIL',))
    ev.evaluate(clusters[:50])                                       # warm: code objects, allocator
    torch.cuda.synchronize()
    split = {}
    t0 = time.perf_counter()
    flat = [tok for c in clusters for tok in c]
    table, tok_off, tok_n = tde.transcribe(flat, a, ('SIL',))
    split['transcription_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    t1, t2 = tde.pair_table(clusters)
    keep = (tok_n[t1] > 0) | (tok_n[t2] > 0)
    t1, t2 = t1[keep], t2[keep]
    split['pair_table_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    dist = tde.edit_distance_batch(table, tok_off[t1], tok_n[t1], table, tok_off[t2], tok_n[t2]).cpu().numpy()
    split['kernel_with_upload_sort_download_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    value = tde.ned(dist, np.maximum(tok_n[t1], tok_n[t2]))
    split['reduction_s'] = time.perf_counter() - t0
    t0 = time.perf_counter()
    s = ev.evaluate(clusters)
    total = time.perf_counter() - t0
    assert s.ned == value and len(s.dist) == len(dist)
    return {'files': n_files, 'phones': int(len(a.ids)), 'clusters': n_clusters, 'tokens': s.n_tokens, 'pairs': s.n_pairs,
            'skipped': s.n_skipped, 'ned': s.ned, 'coverage': s.coverage, 'evaluate_s': round(total, 4),
            'split': {k: round(v, 4) for k, v in split.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=2000000)
    ap.add_argument('--unit-pairs', type=int, default=150607)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tde_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15,
           'shapes': [shape('ned', a.pairs, 40, 1), shape('units', a.unit_pairs, 1024, 2)], 'evaluate': end_to_end()}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
