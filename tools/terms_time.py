"""Times term discovery (abnet3_amd/terms.py) on a synthetic corpus with planted repeats and no audio: utterances of
2-10 s (200-1000 frames of 10 ms), D = 100, smooth random trajectories, a few "words" of 50-90 frames copied (with
noise) into several utterances each.

  abn_dtw_local_batched    the local-alignment kernel alone on TermDiscoverer's own pair table -- every utterance whole
                           against every window of every utterance, windows of 256 frames (device events)
  abn_dtw_search_batched   the search kernel on the SAME pair table (side 1 = the utterance, side 2 = the window as the
                           query: 256 frames is the search's cap, which is why the table is windowed at 256 and not at
                           the local mode's own 512), in the same process.  Its machine code is the parent commit's
                           (the disassembly of search.hip's kernels did not change), so it is the yardstick; the ratio
                           of the two cells/s figures is the figure of record.  The LOCAL kernel is never its own.
  the same at the local mode's cap (windows of 512 frames): LOCAL alone, to show what the longer boundary row costs
  TermDiscoverer.discover  end to end (pair enumeration, upload, kernel, download, filtering, clustering), wall time

--distance kl: the same over a row softmax of the features (abn_dtw_local_kl_batched against abn_dtw_search_kl_batched).

Every GPU route settles the clock (untimed calls for 0.3 s) before its timed calls; medians are reported.
python tools/terms_time.py [--utts N] [--distance cosine|kl] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from abnet3_amd import _lib
from abnet3_amd.terms import TermDiscoverer, kernel_pairs
from tools.abx_time import median_ms, wall


def synthetic(n_utts, n_words=8, D=100, seed=0, noise=0.05):
    """(feats, times, planted {word: [(name, first, last)]}): random walks, renormalised; word w is copied with a little
    noise into utterances w, w + n_words, ... at a random place."""
    rng = np.random.default_rng(seed)

    def walk(n):
        f = np.cumsum(0.35 * rng.standard_normal((n, D)), axis=0) + rng.standard_normal((n, D))
        f -= f.mean(axis=0, keepdims=True)
        return (f / f.std()).astype(np.float32)
    words = [walk(int(rng.integers(50, 91))) for _ in range(n_words)]
    feats, times, planted = {}, {}, {w: [] for w in range(n_words)}
    for u in range(n_utts):
        name = 'utt%04d' % u
        f = walk(int(rng.integers(200, 1001)))
        w = u % n_words
        lo = int(rng.integers(0, len(f) - len(words[w])))
        f[lo:lo + len(words[w])] = words[w] + np.float32(noise) * rng.standard_normal(words[w].shape).astype(np.float32)
        planted[w].append((name, lo, lo + len(words[w]) - 1))
        feats[name], times[name] = f, (np.arange(len(f)) + 0.5) * 0.01
    return feats, times, planted


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=64)
    ap.add_argument('--distance', choices=('cosine', 'kl'), default='cosine')
    ap.add_argument('--theta', type=float, default=None, help='default: 0.25 (cosine), 0.5 (kl); untuned')
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    kl = a.distance == 'kl'
    theta = a.theta if a.theta is not None else (0.5 if kl else 0.25)
    feats, times, planted = synthetic(a.utts)
    if kl:
        feats = {k: torch.softmax(torch.from_numpy(v), dim=1).numpy() for k, v in feats.items()}
    td = TermDiscoverer(feats, times, distance=a.distance, theta=theta)
    c = td.corpus
    rows, D = c.table.shape
    lib = _lib.load()
    ptr = _lib.ptr
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    base = np.array([c.offset[k] for k in td.names], dtype=np.int64)
    length = np.array([c.length[k] for k in td.names], dtype=np.int32)
    n = len(td.names)
    upairs = [(u, v) for u in range(n) for v in range(u, n)]
    table, t = c.table, td.tables

    def pair_table(window):
        kp = np.array(kernel_pairs(length.tolist(), upairs, window), dtype=np.int64)
        o1, n1, o2, n2 = base[kp[:, 0]], length[kp[:, 0]], base[kp[:, 1]] + kp[:, 2], kp[:, 3].astype(np.int32)
        return ([dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)], len(kp),
                int(np.dot(n1.astype(np.int64), n2.astype(np.int64))))

    def outputs(P):
        return [torch.empty(P, dtype=torch.float64, device='cuda')] + [torch.empty(P, dtype=torch.int32, device='cuda') for _ in range(5)]

    def local(tab, P, o):
        out = [float(np.float32(theta)), 0] + [ptr(x) for x in o] + [_lib.stream()]
        if kl:
            _lib.check(lib.abn_dtw_local_kl_batched(ptr(t.P), ptr(t.L), rows, ptr(t.P), ptr(t.L), rows, *[ptr(x) for x in tab],
                                                    P, D, ptr(t.bad), ptr(t.bad), *out), 'abn_dtw_local_kl_batched')
        else:
            _lib.check(lib.abn_dtw_local_batched(ptr(table), rows, ptr(table), rows, *[ptr(x) for x in tab], P, D, *out),
                       'abn_dtw_local_batched')

    def search(tab, P, o):
        out = [ptr(x) for x in o[:4]] + [None, 0, None, None, None, _lib.stream()]
        if kl:
            _lib.check(lib.abn_dtw_search_kl_batched(ptr(t.P), ptr(t.L), rows, ptr(t.P), ptr(t.L), rows, *[ptr(x) for x in tab],
                                                     P, D, ptr(t.bad), ptr(t.bad), *out), 'abn_dtw_search_kl_batched')
        else:
            _lib.check(lib.abn_dtw_search_batched(ptr(table), rows, ptr(table), rows, *[ptr(x) for x in tab], P, D, *out),
                       'abn_dtw_search_batched')

    tab256, P256, cells256 = pair_table(256)
    tab512, P512, cells512 = pair_table(512)
    o256, s256, o512 = outputs(P256), outputs(P256), outputs(P512)
    l_ms = median_ms(lambda: local(tab256, P256, o256), a.calls)
    s_ms = median_ms(lambda: search(tab256, P256, s256), a.calls)
    l_ms2 = median_ms(lambda: local(tab256, P256, o256), a.calls)
    s_ms2 = median_ms(lambda: search(tab256, P256, s256), a.calls)
    w_ms = median_ms(lambda: local(tab512, P512, o512), a.calls)
    torch.cuda.synchronize()
    m0, c0 = td.discover()                                              # warm
    walls = []
    for _ in range(3):
        w, (m, cl) = wall(td.discover)
        walls.append(w)
        assert m == m0 and cl == c0
    number = {k: f for f, k in enumerate(td.names)}
    whole = 0
    for occ in planted.values():                                        # a word counts when one cluster covers all its copies
        want = [(number[k], lo, hi) for k, lo, hi in occ]
        whole += any(all(any(f == g and min(hi, h2) - max(lo, l2) + 1 >= 0.8 * (hi - lo + 1) for g, l2, h2 in cl) for f, lo, hi in want)
                     for cl in c0)
    lname = 'abn_dtw_local_kl_batched' if kl else 'abn_dtw_local_batched'
    sname = 'abn_dtw_search_kl_batched' if kl else 'abn_dtw_search_batched'
    rate = lambda cells, ms: round(cells / (ms * 1e-3), 1)
    res = {
        'device': torch.cuda.get_device_name(0), 'distance': a.distance, 'theta': theta,
        'set': '%d utterances of 200-1000 frames (%d rows), D = %d; %d words of 50-90 frames planted %d times each; every '
               'utterance whole against every window of every utterance (itself included)' % (n, rows, D, len(planted), n // len(planted)),
        'pairs_window_256': P256, 'cells_window_256': cells256, 'pairs_window_512': P512, 'cells_window_512': cells512,
        lname + '_ms_window_256': round(l_ms, 4), lname + '_ms_window_256_again': round(l_ms2, 4),
        lname + '_cells_per_s_window_256': rate(cells256, l_ms),
        sname + '_ms_same_table': round(s_ms, 4), sname + '_ms_same_table_again': round(s_ms2, 4),
        sname + '_cells_per_s': rate(cells256, s_ms),
        'local_over_search_cells_per_s': round(s_ms / l_ms, 3),
        lname + '_ms_window_512': round(w_ms, 4), lname + '_cells_per_s_window_512': rate(cells512, w_ms),
        'discover_end_to_end_s_median': round(float(np.median(walls)), 4),
        'discover_matches': len(m0), 'discover_clusters': len(c0),
        'planted_words_recovered_as_one_cluster': '%d of %d' % (whole, len(planted)),
        'protocol': 'settle 0.3 s of untimed calls, then the median of %d device-event timings per route; the routes '
                    'alternate in one process; the search kernel is the parent commit\'s machine code' % a.calls,
    }
    print(json.dumps(res))
    if a.out:
        merged = {}
        if os.path.exists(a.out):
            with open(a.out) as f:
                merged = json.load(f)
        merged[a.distance] = res
        with open(a.out, 'w') as f:
            json.dump(merged, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
