"""Times the pair-free histogram route of the term scores (abns_edit_cluster_hist, tde.cluster_histogram,
TermEvaluator.evaluate_full) against the pair-table route (tde.pair_table, abn_edit_distance_batched, TermEvaluator.evaluate)
on the same device and clusters.

Workloads, ES-KMeans-shaped and synthetic (nothing measured on real speech): 200 files of 2000 phones of 80 ms over 40
symbols; about 1.5e5 tokens, each a run of whole phones, in 1000 clusters whose sizes fall off like rank^-0.7;
transcriptions of 1 - 12 phones ('short') and of 3 - 30 ('long'); and 'one-type': ONE cluster of 20 000 tokens that all
carry the same six phones, the single-hot-bucket case.  Per workload, the routes alternating in one process, every figure
the median of 15 calls after the clock has settled (tools/gmm_time.py's median_ms: untimed calls for 0.3 s, device events
around each call, which also cover the host work between them):

  hist_entry          abns_edit_cluster_hist alone on device-resident columns already sorted by length: the token check,
                      the wait for it, two memsets and the kernel -- pairs/s is taken from this
  cluster_histogram   tde.cluster_histogram from host columns: uploads, the length sort, the entry, the read-back
  evaluate_full       TermEvaluator.evaluate_full end to end, from the clusters as lists of (file, onset, offset)
  and on a SUBSAMPLE (every seventh cluster while the pairs fit, or for 'one-type' the first tokens, up to about 4e6 pairs -- the pair table of the
  whole workload is gigabytes; the subsample is stated in the output):
  evaluate            TermEvaluator.evaluate end to end
  pair_table_host     tde.pair_table alone (host, perf_counter)
  edit_entry          abn_edit_distance_batched alone on the explicit table of the subsample's pairs, device-resident and
                      sorted as edit_distance_batch sorts it
  hist_entry_sub      abns_edit_cluster_hist alone on the same subsample: the same pairs, with the enumeration, the overlap
                      test and the counting on top of the distance -- what the atomics and the unranking cost
  evaluate_full_sub   evaluate_full on the subsample
torch.cuda.max_memory_allocated over one call of evaluate_full (whole workload) and of evaluate and evaluate_full (subsample).

python tools/tde_full_time.py [--out FILE] [--tokens N]"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, 'tools'))
import numpy as np

from gmm_time import median_ms

N_FILES, N_PHONES, PHONE_S, ALPHABET = 200, 2000, 0.08, 40
SUB_PAIRS = 4000000


def alignment(rng):
    from abnet3_amd import tde
    files = np.repeat(['f%03d' % f for f in range(N_FILES)], N_PHONES)
    k = np.tile(np.arange(N_PHONES), N_FILES)
    sym = ['p%02d' % s for s in rng.integers(0, ALPHABET, N_FILES * N_PHONES)]
    return tde.make_alignment(files, k * PHONE_S, (k + 1) * PHONE_S, sym)


def skewed_sizes(n_tokens, n_clusters):
    w = np.arange(1, n_clusters + 1) ** -0.7
    sizes = np.maximum(1, np.round(w / w.sum() * n_tokens)).astype(np.int64)
    return sizes


def clusters_of(rng, sizes, lo, hi):
    out = []
    for s in sizes:
        f = rng.integers(0, N_FILES, s)
        n = rng.integers(lo, hi + 1, s)
        k = rng.integers(0, N_PHONES - hi, s)
        out.append([('f%03d' % a, b * PHONE_S, (b + c) * PHONE_S) for a, b, c in zip(f.tolist(), k.tolist(), n.tolist())])
    return out


def one_type_cluster(a, n_tokens):
    """n_tokens tokens that all carry the six phones of file 0's first six rows: every file gets the same six phones there."""
    ids = a.ids.copy()
    for f in range(N_FILES):
        for r in range(0, N_PHONES - 6, 6):
            ids[a.first[f] + r:a.first[f] + r + 6] = ids[:6]
    a = a._replace(ids=ids)
    per = -(-n_tokens // N_FILES)
    toks = [('f%03d' % f, 6 * r * PHONE_S, (6 * r + 6) * PHONE_S) for f in range(N_FILES) for r in range(per)][:n_tokens]
    return a, [toks]


def host_ms(fn, calls=15):
    fn()
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append(1e3 * (time.perf_counter() - t0))
    return {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(float(min(ts)), 3), 'max_ms': round(float(max(ts)), 3)}


def peak_bytes(fn):
    import torch
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    before = torch.cuda.memory_allocated()
    fn()
    torch.cuda.synchronize()
    return int(torch.cuda.max_memory_allocated() - before)


def n_pairs_of(clusters):
    return int(sum(len(c) * (len(c) - 1) // 2 for c in clusters))


def subsample(clusters):
    if len(clusters) == 1:
        n = int((2 * SUB_PAIRS) ** 0.5)
        return [clusters[0][:n]], 'the first %d tokens of the cluster' % n
    out, total = [], 0
    for c in clusters[::7]:                                         # every seventh cluster, while the pairs fit
        if total + len(c) * (len(c) - 1) // 2 <= SUB_PAIRS:
            out.append(c)
            total += len(c) * (len(c) - 1) // 2
    return out, 'every seventh cluster that still fits under %d pairs: %d of %d clusters' % (SUB_PAIRS, len(out), len(clusters))


def hist_entry(ev, clusters):
    """(callable that runs abns_edit_cluster_hist alone on sorted device columns, the pairs it counts)."""
    import torch
    from abnet3_amd import _lib
    lib = _lib.load()
    _, s, tok_file, tok_on, tok_end, cl_first, _, _ = ev.prepare_full(clusters)
    cid = np.repeat(np.arange(len(cl_first) - 1), np.diff(cl_first))
    order = np.lexsort((s.tok_n, cid))
    cols = [torch.from_numpy(np.ascontiguousarray(c[order])).cuda() for c in (s.tok_off, s.tok_n, tok_file, tok_on, tok_end)]
    table = torch.from_numpy(s.table).cuda()
    M = max(1, int(s.tok_n.max()))
    hist = torch.empty((2, M + 1, M + 1), dtype=torch.int64, device='cuda')
    counts = torch.empty(2, dtype=torch.int64, device='cuda')
    n_ws = int(lib.abns_edit_cluster_hist_ws_bytes(len(s.tok_n), len(cl_first) - 1, 0))
    ws = torch.empty(n_ws, dtype=torch.uint8, device='cuda')

    def run():
        _lib.check(lib.abns_edit_cluster_hist(_lib.ptr(table), table.numel(), *[_lib.ptr(c) for c in cols], None, len(s.tok_n),
                                              cl_first.ctypes.data, len(cl_first) - 1, M, _lib.ptr(hist), _lib.ptr(counts), _lib.ptr(ws), n_ws,
                                              _lib.stream()), 'abns_edit_cluster_hist')
    run()
    return run, int(counts.cpu()[0]), (s, tok_file, tok_on, tok_end, cl_first)


def edit_entry(ev, clusters):
    """(callable that runs abn_edit_distance_batched alone on the sorted explicit pair table, its pairs, the table's bytes)."""
    import torch
    from abnet3_amd import _lib
    lib = _lib.load()
    _, _, (table, tok_off, tok_n), (t1, t2), _, _, _ = ev.prepare(clusters)
    n1, n2 = tok_n[t1], tok_n[t2]
    order = np.lexsort((np.maximum(n1, n2), np.minimum(n1, n2)))
    cols = [torch.from_numpy(np.ascontiguousarray(c[order])).cuda() for c in (tok_off[t1], n1, tok_off[t2], n2)]
    sym = torch.from_numpy(table).cuda()
    dist = torch.empty(len(t1), dtype=torch.int32, device='cuda')
    max_short = int(max(1, np.minimum(n1, n2).max()))

    def run():
        _lib.check(lib.abn_edit_distance_batched(_lib.ptr(sym), sym.numel(), _lib.ptr(sym), sym.numel(), *[_lib.ptr(c) for c in cols], len(t1),
                                                 max_short, _lib.ptr(dist), _lib.stream()), 'abn_edit_distance_batched')
    run()
    return run, len(t1), int(sum(c.numel() * c.element_size() for c in cols) + dist.numel() * 4)


def rate(pairs, t):
    return round(pairs / (t['median_ms'] * 1e-3), 0)


def workload(name, a, clusters, ignore=()):
    from abnet3_amd import tde
    ev = tde.TermEvaluator(a, ignore=ignore)
    res = {'name': name, 'n_tokens': int(sum(len(c) for c in clusters)), 'n_clusters': len(clusters), 'same_cluster_pairs': n_pairs_of(clusters)}
    run_hist, pairs, (s, tok_file, tok_on, tok_end, cl_first) = hist_entry(ev, clusters)
    res.update(pairs_after_the_overlap_rule=pairs, longest_transcription=int(s.tok_n.max()),
               pair_table_bytes_of_the_whole_workload=24 * n_pairs_of(clusters))
    sub, how = subsample(clusters)
    run_hist_sub, pairs_sub, _ = hist_entry(ev, sub)
    run_edit, pairs_edit, table_bytes = edit_entry(ev, sub)
    res['subsample'] = {'what': how, 'n_tokens': int(sum(len(c) for c in sub)), 'pairs_after_the_overlap_rule': pairs_sub,
                        'scored_pairs_in_the_table': pairs_edit, 'device_bytes_of_the_table_and_its_result': table_bytes}
    full_out = {}

    def full():
        full_out['s'] = ev.evaluate_full(clusters)

    res['hist_entry'] = median_ms(run_hist)
    res['cluster_histogram'] = median_ms(lambda: tde.cluster_histogram(s.table, s.tok_off, s.tok_n, tok_file, tok_on, tok_end, cl_first))
    res['evaluate_full'] = median_ms(full)
    res['edit_entry'] = median_ms(run_edit)
    res['hist_entry_sub'] = median_ms(run_hist_sub)
    res['evaluate'] = median_ms(lambda: ev.evaluate(sub))
    res['evaluate_full_sub'] = median_ms(lambda: ev.evaluate_full(sub))
    res['pair_table_host'] = host_ms(lambda: tde.pair_table(sub))
    res['hist_entry_again'] = median_ms(run_hist)                      # (alternating: the kernel once more)
    res['hist_entry']['pairs_per_s'] = rate(pairs, res['hist_entry'])
    res['hist_entry_sub']['pairs_per_s'] = rate(pairs_sub, res['hist_entry_sub'])
    res['edit_entry']['pairs_per_s'] = rate(pairs_edit, res['edit_entry'])
    res['hist_over_edit_time_on_the_same_pairs'] = round(res['hist_entry_sub']['median_ms'] / res['edit_entry']['median_ms'], 3)
    res['peak_device_bytes'] = {'evaluate_full': peak_bytes(full), 'evaluate_full_sub': peak_bytes(lambda: ev.evaluate_full(sub)),
                                'evaluate_sub': peak_bytes(lambda: ev.evaluate(sub))}
    old, new = ev.evaluate(sub), ev.evaluate_full(sub)
    res['agreement_on_the_subsample'] = {'ned_evaluate': old.ned, 'ned_evaluate_full': new.ned, 'n_pairs_equal': old.n_pairs == new.n_pairs,
                                         'n_skipped_equal': old.n_skipped == new.n_skipped}
    res['scores'] = {'ned': full_out['s'].ned, 'grouping': list(full_out['s'].grouping), 'n_same': full_out['s'].n_same}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'tde_full_time.json'))
    ap.add_argument('--tokens', type=int, default=150000)
    args = ap.parse_args()
    import torch
    rng = np.random.default_rng(0)
    a = alignment(rng)
    sizes = skewed_sizes(args.tokens, 1000)
    one_a, one = one_type_cluster(a, 20000)
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'note': 'synthetic clusters: nothing measured on real speech',
           'workloads': [workload('short', a, clusters_of(rng, sizes, 1, 12)), workload('long', a, clusters_of(rng, sizes, 3, 30)),
                         workload('one-type', one_a, one)]}
    print(json.dumps(res))
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
