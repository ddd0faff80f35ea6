"""Times the segment kNN search (abnet3_amd/csrc/knn.hip) and the pair miner (abnet3_amd/discovery.py).

  abn_knn_topk             nq = nc = 2^17 unit vectors, d = 400, k = 10, the overlap exclusion on (files of 512
                           segments, begins 5 apart, lengths 40 / 60 / 80), one call = search + merge (device events)
  torch composition        the same search with what the library offered before this kernel: per chunk of queries a
                           torch.mm against the whole table, the exclusion as a broadcast mask, torch.topk; same
                           tables, same GPU, same run
  KnnPairMiner             end to end on tools/c5_corpus.py's corpus (filterbanks of --utts utterances): wall time and
                           its phases (segment vectors, neighbour lists, pair list, files)

Every GPU route settles the clock (untimed calls for 0.3 s) before its 15 timed calls; medians are reported.  The
roofline is 2 nq nc d flops against the fp32 matrix-core rate (157.3 TFLOP/s: 64 flop / clock / SIMD, 1024 SIMDs,
2.4 GHz).  One run writes one JSON; `--merge run1.json run2.json run3.json` folds three runs into
profiles/knn_time.json with the spread of both medians over the runs.

python tools/knn_time.py [--log2n 17] [--utts 200] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FP32_MFMA_FLOPS = 157.3e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


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
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def torch_search(table, meta, k, chunk):
    """The composition: chunked mm + mask + topk."""
    import torch
    f, b, e = meta[:, 0], meta[:, 1], meta[:, 2]
    idx, sim = [], []
    for q0 in range(0, table.shape[0], chunk):
        q1 = min(table.shape[0], q0 + chunk)
        S = torch.mm(table[q0:q1], table.t())
        excl = (f[q0:q1, None] == f[None, :]) & (b[q0:q1, None] < e[None, :]) & (b[None, :] < e[q0:q1, None])
        S.masked_fill_(excl, float('-inf'))
        s, i = torch.topk(S, k, dim=1)
        idx.append(i)
        sim.append(s)
    return torch.cat(idx), torch.cat(sim)


def run(a):
    import torch
    from abnet3_amd import _lib
    from abnet3_amd.discovery import KnnPairMiner, knn_topk, pairs_from_lists
    n, d, k = 1 << a.log2n, 400, 10
    g = torch.Generator(device='cuda').manual_seed(0)
    table = torch.randn(n, d, device='cuda', generator=g)
    table = (table / table.norm(dim=1, keepdim=True)).contiguous()
    seg = torch.arange(n, device='cuda')
    begin = (seg % 512) * 5
    meta = torch.stack([seg // 512, begin, begin + 40 + 20 * (seg % 3)], dim=1).to(torch.int32).contiguous()
    res = {'device': torch.cuda.get_device_name(0), 'nq': n, 'nc': n, 'd': d, 'k': k,
           'flops_per_call': 2.0 * n * n * d, 'calls_per_median': 15}
    hold = {}

    def fused():
        hold['fused'] = knn_topk(table, table, k, meta, meta)

    def composed():
        hold['torch'] = torch_search(table, meta, k, a.chunk)

    f_ms, f_lo, f_hi = median_ms(fused)
    c_ms, c_lo, c_hi = median_ms(composed)
    same_rows = float((hold['fused'][0].long() == hold['torch'][0]).all(dim=1).float().mean())
    max_dsim = float((hold['fused'][1] - hold['torch'][1]).abs().max())
    lib = _lib.load()
    res['abn_knn_topk'] = {'median_ms': round(f_ms, 3), 'min_ms': round(f_lo, 3), 'max_ms': round(f_hi, 3),
                           'tflops': round(res['flops_per_call'] / (f_ms * 1e-3) / 1e12, 2),
                           'fraction_of_fp32_mfma_roof': round(res['flops_per_call'] / (f_ms * 1e-3) / FP32_MFMA_FLOPS, 4),
                           'workspace_bytes': int(lib.abn_knn_ws_bytes(n, n, k))}
    res['torch_mm_mask_topk'] = {'median_ms': round(c_ms, 3), 'min_ms': round(c_lo, 3), 'max_ms': round(c_hi, 3),
                                 'query_chunk': a.chunk}
    res['speedup_over_torch'] = round(c_ms / f_ms, 3)
    res['agreement'] = {'rows_with_identical_index_lists': round(same_rows, 6), 'max_abs_similarity_difference': max_dsim}
    del hold, table, meta
    torch.cuda.empty_cache()

    # the miner end to end on the C5 corpus' filterbanks
    sys.path.insert(0, os.path.join(ROOT, 'tools'))
    from c5_corpus import synth_corpus
    from abnet3_amd.dataloader import DeviceCorpus
    from abnet3_amd.features import FeaturesGenerator
    corpus = synth_corpus(n_utts=a.utts, seed=0, device='cuda')
    fg = FeaturesGenerator(norm_per_channel=True)
    fb = {name: fg.fbank_from_samples(w, 16000).cpu().numpy() for name, w in zip(corpus.names, corpus.waves)}
    fb, _ = fg.normalize_features(fb)
    dc = DeviceCorpus(fb, {name: np.arange(len(v)) * 0.01 + 0.0125 for name, v in fb.items()})

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0, out

    out_dir = tempfile.mkdtemp(prefix='knn_time_')
    KnnPairMiner(dc).write(out_dir)                                      # warm
    totals, phases = [], None
    for _ in range(3):
        m = KnnPairMiner(dc)
        t_vec, _ = wall(m.vectors)
        t_knn, _ = wall(m.neighbours)
        t_pairs, m.pairs = wall(lambda: pairs_from_lists(m.idx, m.sim, m.min_similarity, m.mutual, m.max_pairs))
        t_write, _ = wall(lambda: m.write(out_dir))
        totals.append(t_vec + t_knn + t_pairs + t_write)
        phases = {'segment_vectors': round(t_vec, 4), 'neighbour_lists': round(t_knn, 4), 'pair_list_host': round(t_pairs, 4),
                  'write_files': round(t_write, 4)}
    res['miner_on_c5_corpus'] = {'utterances': a.utts, 'frames': int(dc.total), 'feature_dim': int(dc.dim),
                                 'segments': int(m.table.shape[0]), 'vector_dim': int(m.table.shape[1]),
                                 'pairs': int(len(m.pairs[0])), 'end_to_end_s_median': round(float(np.median(totals)), 4),
                                 'phase_s_last_run': phases}
    return res


def merge(paths, out):
    runs = [json.load(open(p)) for p in paths]
    f = [r['abn_knn_topk']['median_ms'] for r in runs]
    c = [r['torch_mm_mask_topk']['median_ms'] for r in runs]
    res = dict(runs[-1])
    res['runs'] = len(runs)
    res['abn_knn_topk_median_ms_per_run'] = f
    res['torch_mm_mask_topk_median_ms_per_run'] = c
    res['spread_ms'] = {'abn_knn_topk': round(max(f) - min(f), 3), 'torch_mm_mask_topk': round(max(c) - min(c), 3)}
    res['speedup_over_torch_per_run'] = [round(y / x, 3) for x, y in zip(f, c)]
    res['gap_ms_smallest'] = round(min(c) - max(f), 3)
    res['faster_by_more_than_the_spread'] = bool(min(c) - max(f) > (max(f) - min(f)) + (max(c) - min(c)))
    res['miner_end_to_end_s_per_run'] = [r['miner_on_c5_corpus']['end_to_end_s_median'] for r in runs]
    with open(out, 'w') as fh:
        fh.write(json.dumps(res, indent=1) + '\n')
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--log2n', type=int, default=17)
    ap.add_argument('--chunk', type=int, default=4096, help="query rows per torch.mm of the composition")
    ap.add_argument('--utts', type=int, default=200)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'knn_time.json'))
    ap.add_argument('--merge', nargs='+', default=None)
    a = ap.parse_args()
    if a.merge:
        return merge(a.merge, a.out)
    res = run(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
