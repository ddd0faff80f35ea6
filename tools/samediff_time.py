"""Times the same-different kernels (abn_sd_collect, abn_sd_count, abnet3_amd/csrc/samediff.hip) and the table
route around them (abnet3_amd/samediff.py).

Tables: unit vectors, d = 400, tokens = a unit type centre plus `noise` times a unit-scale Gaussian, normalised
(noise 1: same-type cosines near 0.5, different-type ones within a few 1 / sqrt(d) of 0 -- most pairs are less
similar than every positive; noise 2: the populations meet, AP well below 1; noise 4: they overlap and nearly every
pair needs the search and an inner-bucket atomic).  n = 11 000 with types of 19 tokens (P about 10^5) and n = 60 888
with types of 34 (P about 10^6).

  abn_sd_collect, abn_sd_count   one call each through the C ABI (device events; count includes its two clears)
  sort                           torch.sort of the collected list, descending
  table route                    samediff.vector_histogram + scores_from_histogram on the prebuilt table, wall clock
  evaluate                       SameDifferentEvaluator(...).evaluate('vectors') end to end, wall clock: the table's rows
                                 laid out as one file of 10-frame tokens of 40-d frames, so that it also pays the token
                                 lookup (the constructor, timed apart), abn_segment_vectors, the sort by type and the gather
  (a) torch composition          what the library offered before: per chunk of rows a torch.mm against the table, the
                                 upper-triangle mask, torch.searchsorted, torch.bincount; the same thresholds; its
                                 integer histogram is compared with the kernel's bucket by bucket.  Timed twice: as
                                 stated, and with the two end buckets counted by comparison before the bincount (a
                                 bucket that takes most of the pool serialises torch.bincount's atomics)
  (b) floor                      half of abn_knn_topk(k = 1) on the same table: that kernel forms the full square
                                 with the same tile

Every route settles the clock (untimed calls for 0.3 s) before its timed calls; medians of 15 calls (of --torch-calls,
default 3, for the torch compositions; ONE call where a call takes more than 5 s).  Peak allocations are torch's, per
route.  The two histograms must hold the same total (asserted); the buckets that differ are reported.  A run replaces
the tables it measured in the output file and keeps the others, so the file may hold tables of several runs of one
build (each table carries its run's time stamp).

python tools/samediff_time.py [--tables 11000:2,60888:2,11000:1,60888:1,11000:4] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32_MFMA_FLOPS = 157.3e12
TYPE_SIZE = {11000: 19, 60888: 34}


def settle(fn, seconds=0.3):
    import torch
    t0 = time.perf_counter()
    while time.perf_counter() - t0 < seconds:
        fn()
        torch.cuda.synchronize()


def median_ms(fn, calls=15):
    import torch
    settle(fn)
    ts = []
    for _ in range(calls):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1))
    return {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(float(min(ts)), 3), 'max_ms': round(float(max(ts)), 3),
            'calls': calls}


def torch_ms(fn, calls):
    """median_ms of `calls` calls, or the one warm-up call itself when it takes more than 5 s."""
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    torch.cuda.synchronize()
    first = e0.elapsed_time(e1)
    if first > 5000.0:
        return {'median_ms': round(first, 3), 'min_ms': round(first, 3), 'max_ms': round(first, 3), 'calls': 1}
    return median_ms(fn, calls)


def evaluate_end_to_end(X, cbeg):
    """SameDifferentEvaluator over the table's rows as 10-frame tokens of one file: (constructor s, evaluate s, result)."""
    import torch
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.samediff import SameDifferentEvaluator
    n, frames = X.shape[0], 10
    times = np.arange(n * frames) * 0.01
    corpus = DeviceCorpus.from_table(X.view(n * frames, X.shape[1] // frames), ['all'], [n * frames], {'all': times})
    classes, cur = [], None
    for k in range(n):
        if cur is None or cbeg[k] == k:
            cur = []
            classes.append(cur)
        cur.append(('all', float(times[frames * k]), float(times[frames * k + frames - 1])))
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    ev = SameDifferentEvaluator(classes, corpus)
    t1 = time.perf_counter()
    r = ev.evaluate('vectors', frames=frames)
    torch.cuda.synchronize()
    return t1 - t0, time.perf_counter() - t1, r


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - base), out


def make_table(n, size, d, noise, seed):
    import torch
    g = torch.Generator(device='cuda').manual_seed(seed)
    n_types = (n + size - 1) // size
    centre = torch.randn(n_types, d, device='cuda', generator=g)
    centre = centre / centre.norm(dim=1, keepdim=True)
    types = torch.arange(n, device='cuda') // size
    X = centre[types] + noise * torch.randn(n, d, device='cuda', generator=g) / d ** 0.5
    X = (X / X.norm(dim=1, keepdim=True)).contiguous()
    beg = (np.arange(n) // size) * size
    return X, beg.astype(np.int32), np.minimum(beg + size, n).astype(np.int32)


def torch_histogram(X, thr_asc, chunk, ends_apart=False):
    """The composition: chunked mm + upper-triangle mask + searchsorted + bincount; b(x) = P - #{thr <= x}.
    torch.bincount adds with one atomic per element, so a bucket that takes most of the pool serialises it;
    ends_apart counts the two end buckets by comparison first and bins only the pairs between the extreme thresholds."""
    import torch
    n, P = X.shape[0], thr_asc.numel()
    hist = torch.zeros(P + 1, dtype=torch.int64, device=X.device)
    cols = torch.arange(n, device=X.device)
    for r0 in range(0, n, chunk):
        r1 = min(n, r0 + chunk)
        S = torch.mm(X[r0:r1], X[r0:].t())                           # columns r0 .. n - 1: nothing left of the diagonal block
        x = S[cols[None, r0:] > cols[r0:r1, None]]
        if ends_apart:
            low, high = x < thr_asc[0], x >= thr_asc[-1]
            hist[P] += low.sum()
            hist[0] += high.sum()
            x = x[~(low | high)]
        hist += torch.bincount(P - torch.searchsorted(thr_asc, x, right=True), minlength=P + 1)
    return hist


def run_table(n, noise, a):
    import torch
    from abnet3_amd import _lib, samediff
    from abnet3_amd.discovery import knn_topk
    lib = _lib.load()
    d = 400
    X, cbeg, cend = make_table(n, TYPE_SIZE.get(n, 19), d, noise, seed=n)
    d_beg, d_end = torch.from_numpy(cbeg).cuda(), torch.from_numpy(cend).cuda()
    pos_off, total = samediff.positive_offsets(cbeg, cend)
    d_off = torch.from_numpy(pos_off).cuda()
    pos_sim = torch.empty(total, dtype=torch.float32, device='cuda')
    pairs = n * (n - 1) // 2
    res = {'n': n, 'd': d, 'noise': noise, 'pairs': pairs, 'positives': total, 'flops_upper_triangle': 2.0 * pairs * d}

    def collect():
        _lib.check(lib.abn_sd_collect(_lib.ptr(X), n, d, _lib.ptr(d_beg), _lib.ptr(d_end), _lib.ptr(d_off), _lib.ptr(pos_sim),
                                      _lib.stream()), 'abn_sd_collect')
    res['abn_sd_collect'] = median_ms(collect)
    hold = {}

    def sort():
        hold['thr'] = torch.sort(pos_sim, descending=True)[0]
    res['sort'] = median_ms(sort)
    thr = hold['thr']
    hist = torch.empty(total + 1, dtype=torch.int64, device='cuda')
    bad = torch.empty(1, dtype=torch.int64, device='cuda')

    def count():
        _lib.check(lib.abn_sd_count(_lib.ptr(X), n, d, _lib.ptr(d_beg), _lib.ptr(d_end), None, 0, _lib.ptr(thr), total,
                                    _lib.ptr(hist), _lib.ptr(bad), _lib.stream()), 'abn_sd_count')
    res['abn_sd_count'] = median_ms(count)
    ms = res['abn_sd_count']['median_ms']
    res['abn_sd_count']['fraction_of_fp32_mfma_roof'] = round(res['flops_upper_triangle'] / (ms * 1e-3) / FP32_MFMA_FLOPS, 4)
    res['inner_bucket_share'] = round(1.0 - float(hist[0] + hist[-1]) / pairs, 6)
    res['n_bad'] = int(bad.item())
    print('n = %d, noise %g: collect %.3f ms, sort %.3f ms, count %.3f ms, inner buckets %.4f'
          % (n, noise, res['abn_sd_collect']['median_ms'], res['sort']['median_ms'], ms, res['inner_bucket_share']), flush=True)

    def knn():
        hold['knn'] = knn_topk(X, X, 1)
    res['abn_knn_topk_k1'] = median_ms(knn)
    res['floor_ms_half_knn_k1'] = round(res['abn_knn_topk_k1']['median_ms'] / 2, 3)
    res['count_over_floor'] = round(ms / res['floor_ms_half_knn_k1'], 3)
    hold.pop('knn')

    # the table route end to end, wall clock
    walls, parts = [], None
    for _ in range(3):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        t, h, nb = samediff.vector_histogram(X, cbeg, cend)
        h = h.cpu().numpy()
        t1 = time.perf_counter()
        s = samediff.scores_from_histogram(t, h)
        t2 = time.perf_counter()
        walls.append(t2 - t0)
        parts = {'device_route_s': round(t1 - t0, 4), 'scores_host_s': round(t2 - t1, 4)}
    res['table_route'] = {'wall_s_median': round(float(np.median(walls)), 4), 'last_run': parts, 'ap': s.ap, 'prb': s.prb}
    res['kernel_route_peak_bytes'] = peak_bytes(lambda: samediff.vector_histogram(X, cbeg, cend))[0]
    evaluate_end_to_end(X, cbeg)                                         # warm
    t_init, t_eval, r = evaluate_end_to_end(X, cbeg)
    assert r.n_tokens == n and r.n_positives == total and abs(r.ap - s.ap) < 1e-3, (r, s.ap)
    res['evaluate_end_to_end'] = {'constructor_s': round(t_init, 4), 'evaluate_s': round(t_eval, 4), 'ap': r.ap, 'prb': r.prb}
    print('n = %d: knn(k = 1) %.3f ms, table route %.3f s, evaluate %.3f s behind a constructor of %.3f s, AP %.4f'
          % (n, res['abn_knn_topk_k1']['median_ms'], res['table_route']['wall_s_median'], t_eval, t_init, s.ap), flush=True)

    # (a) the torch composition on the same thresholds
    thr_asc = torch.flip(thr, [0]).contiguous()
    res['torch_peak_bytes'], t_hist = peak_bytes(lambda: torch_histogram(X, thr_asc, a.chunk))
    res['torch_mm_searchsorted_bincount'] = torch_ms(lambda: torch_histogram(X, thr_asc, a.chunk), a.torch_calls)
    res['torch_mm_searchsorted_bincount']['row_chunk'] = a.chunk
    res['torch_ends_apart'] = torch_ms(lambda: torch_histogram(X, thr_asc, a.chunk, True), a.torch_calls)
    assert bool((torch_histogram(X, thr_asc, a.chunk, True) == t_hist).all())
    res['speedup_over_torch_ends_apart'] = round(res['torch_ends_apart']['median_ms'] / ms, 3)
    assert int(t_hist.sum()) == int(hist.sum()), (int(t_hist.sum()), int(hist.sum()))     # the same pool, whatever the buckets
    differ = int((t_hist != hist).sum())
    res['buckets_that_differ_from_torch'] = {'count': differ, 'share': round(differ / (total + 1), 6),
                                             'pairs_moved': int((t_hist - hist).abs().sum() // 2),
                                             'totals_equal': bool(int(t_hist.sum()) == int(hist.sum()))}
    res['speedup_over_torch'] = round(res['torch_mm_searchsorted_bincount']['median_ms'] / ms, 3)
    print('n = %d: torch composition %.3f ms (x %.2f), ends apart %.3f ms (x %.2f), %d of %d buckets differ' % (
        n, res['torch_mm_searchsorted_bincount']['median_ms'], res['speedup_over_torch'], res['torch_ends_apart']['median_ms'],
        res['speedup_over_torch_ends_apart'], differ, total + 1), flush=True)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--tables', default='11000:2,60888:2,11000:1,60888:1,11000:4', help='n:noise, comma separated')
    ap.add_argument('--chunk', type=int, default=2048, help='rows per torch.mm of the composition')
    ap.add_argument('--torch-calls', type=int, default=3, help='timed calls of each torch composition (one call can take seconds)')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'samediff_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'tables': []}
    if a.out and os.path.exists(a.out):                     # tables of earlier runs stay until they are measured again
        res['tables'] = json.load(open(a.out)).get('tables', [])
    stamp = time.strftime('%Y-%m-%d %H:%M:%S')
    for spec in a.tables.split(','):
        n, noise = int(spec.split(':')[0]), float(spec.split(':')[1])
        table = dict(run_table(n, noise, a), run=stamp)
        res['tables'] = [t for t in res['tables'] if (t['n'], t['noise']) != (n, noise)] + [table]
        if a.out:                                           # after every table: a partial file beats none
            os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
            with open(a.out, 'w') as fh:
                fh.write(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res))


if __name__ == '__main__':
    main()
