"""Times the pair sampler (abnet3_amd/sampler.py, abnet3_amd/csrc/sampler.hip).

  abn_sample_pairs     500 000 pairs (pair_counts(500000, 0.5, 0.5): buckeye.yaml's ratios) on a C5-sized cluster
                       set -- 2000 utterances of 2-10 s, 600 Zipfian word types as tools/c5_corpus.py draws them, 40
                       speakers of 50 utterances -- device events around ONE call of the entry point with
                       preallocated outputs: the launch as a caller sees it (at these sizes the interval holds the
                       host's issue of the launch as well as the kernel), not a kernel-trace figure
  build_tables         host time to build the O(cells) tables from the description; their upload
  sample()             end to end from the .classes / spkid files to both pair directories (wall)
  explicit table       on a cluster set small enough for it (--small-types types, 6 speakers): the only route there
                       was before -- explicit_table for the four configurations (built on the host, timed) sampled
                       with torch.multinomial on the same GPU in the same run -- against build_tables + the kernel on
                       the same set

Every GPU route settles the clock (untimed calls for 0.3 s) before its 15 timed calls; medians are reported.

python tools/sampler_time.py [--pairs 500000] [--out FILE]"""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

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
    return round(float(np.median(ts)), 4), round(float(min(ts)), 4), round(float(max(ts)), 4)


def median_wall_ms(fn, calls=15):
    ts = []
    for _ in range(calls):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(ts)), 3)


def cluster_set(n_utts, n_types, n_spk, seed=0):
    """Clusters (one per word type in use) of [file, onset, offset] tokens and {file: speaker}: utterances of 2-10 s
    filled with Zipfian word tokens of 0.3-1.0 s, tools/c5_corpus.py's statistics without the audio."""
    rng = np.random.default_rng(seed)
    dur = rng.uniform(0.3, 1.0, n_types)
    zipf = 1.0 / np.arange(1, n_types + 1)
    zipf /= zipf.sum()
    by_type = [[] for _ in range(n_types)]
    spk_of = {}
    for u in range(n_utts):
        name = 'utt%05d' % u
        spk_of[name] = 'spk%03d' % (u % n_spk)
        target, pos = rng.uniform(2.0, 10.0), 0.0
        while True:
            gap, w = rng.uniform(0.03, 0.15), int(rng.choice(n_types, p=zipf))
            n = dur[w] * rng.uniform(0.85, 1.15)
            if pos + gap + n > target and pos > 0:
                break
            by_type[w].append([name, round(pos + gap + 0.01, 2), round(pos + gap + n - 0.01, 2)])
            pos += gap + n
    return [c for c in by_type if c], spk_of


def write_files(clusters, spk_of, folder):
    std, spk = os.path.join(folder, 'words.classes'), os.path.join(folder, 'wav2spk.lst')
    with open(std, 'w') as fh:
        for t, c in enumerate(clusters):
            fh.write('Class %d\n' % t + ''.join('%s %.2f %.2f\n' % tuple(tok) for tok in c) + '\n')
    with open(spk, 'w') as fh:
        fh.write(''.join('%s %s\n' % kv for kv in spk_of.items()))
    return std, spk


def run(a):
    import torch
    from abnet3_amd import sampler as S
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15}
    sam = S.SamplerClusterSiamese(ratio_same_diff_spk=0.5)
    counts = S.pair_counts(a.pairs, 0.5, 0.5)
    n = [counts[c] for c in S.CONFIGS]

    clusters, spk_of = cluster_set(a.utts, a.types, a.speakers)
    descr = sam.analyze_clusters(clusters, spk_of)
    tables = S.build_tables(descr)
    dev = S.DeviceTables(tables)
    out = (torch.empty(2, sum(n), dtype=torch.int32, device='cuda'), torch.empty(sum(n), dtype=torch.int64, device='cuda'))
    k_ms = median_ms(lambda: S.sample_pairs_device(dev, n, 0, out=out))
    res['c5_sized'] = {'utterances': a.utts, 'types': len(clusters), 'speakers': a.speakers, 'tokens': len(descr['tokens']),
                       'cells': int(tables['n_cells']), 'pairs': int(sum(n)), 'table_bytes': int(dev.nbytes),
                       'abn_sample_pairs_call_ms': dict(zip(('median', 'min', 'max'), k_ms)),
                       'pairs_per_s': round(sum(n) / (k_ms[0] * 1e-3), 0),
                       'build_tables_host_ms': median_wall_ms(lambda: S.build_tables(descr)),
                       'upload_tables_ms': median_wall_ms(lambda: (S.DeviceTables(tables), torch.cuda.synchronize())),
                       'draw_pairs_ms': median_wall_ms(lambda: S.draw_pairs(descr, counts, 'log', 'log', 0), calls=5)}
    folder = tempfile.mkdtemp(prefix='sampler_time_')
    std, spk = write_files(clusters, spk_of, folder)
    walls = []
    for r in range(3):
        s = S.SamplerClusterSiamese(std_file=std, spkid_file=spk, directory_output=os.path.join(folder, 'pairs%d' % r),
                                    num_total_sampled_pairs=a.pairs, ratio_same_diff_spk=0.5, max_size_cluster=20)
        t0 = time.perf_counter()
        s.sample()
        walls.append(time.perf_counter() - t0)
    res['c5_sized']['sample_end_to_end_s'] = round(float(np.median(walls)), 3)

    # the explicit table, where it fits
    clusters, spk_of = cluster_set(a.small_utts, a.small_types, 6, seed=1)
    descr = sam.analyze_clusters(clusters, spk_of)
    t0 = time.perf_counter()
    explicit = [S.explicit_table(descr, c) for c in S.CONFIGS]
    t_table = time.perf_counter() - t0
    probs = [torch.from_numpy(p).cuda() for _, p in explicit]

    def multinomial():
        return [torch.multinomial(p, m, replacement=True) for p, m in zip(probs, n) if len(p) and m]
    m_ms = median_ms(multinomial)
    tables = S.build_tables(descr)
    dev = S.DeviceTables(tables)
    s_ms = median_ms(lambda: S.sample_pairs_device(dev, n, 0, out=out))
    res['small'] = {'types': len(clusters), 'speakers': 6, 'tokens': len(descr['tokens']), 'cells': int(tables['n_cells']),
                    'keys': [len(k) for k, _ in explicit], 'pairs': int(sum(n)),
                    'explicit_table_build_host_s': round(t_table, 3),
                    'torch_multinomial_ms': dict(zip(('median', 'min', 'max'), m_ms)),
                    'explicit_route_total_ms': round(t_table * 1e3 + m_ms[0], 3),
                    'build_tables_host_ms': median_wall_ms(lambda: S.build_tables(descr)),
                    'abn_sample_pairs_call_ms': dict(zip(('median', 'min', 'max'), s_ms))}
    res['small']['table_route_total_ms'] = round(res['small']['build_tables_host_ms'] + s_ms[0], 3)
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--pairs', type=int, default=500000)
    ap.add_argument('--utts', type=int, default=2000)
    ap.add_argument('--types', type=int, default=600)
    ap.add_argument('--speakers', type=int, default=40)
    ap.add_argument('--small-utts', type=int, default=120)
    ap.add_argument('--small-types', type=int, default=60)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'sampler_time.json'))
    a = ap.parse_args()
    res = run(a)
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
