"""Times the prefilter of term discovery (abnet3_amd/prefilter.py) on tools/terms_time.py's synthetic corpus (64
utterances of 200-1000 frames, D = 100, words of 50-90 frames copied with noise) and TermDiscoverer's own pair table.

  abn_lsh_signatures          64 bits over the corpus table (which fits the last-level cache: replayed calls read it from
                              there) and over a table of 1.14 M rows x 100 (456 MB, beyond every cache); the fraction of
                              the HBM bound of ONE read of the table (8.0 TB/s peak, 6.29 TB/s measured copy)
  abn_lsh_diag_hits_batched   cells/s against abn_dtw_local_batched's on the SAME pair table in the same process, the two
                              alternating; the local kernel is the parent commit's machine code, so it is the yardstick
                              and the ratio is the figure of record.  Windows of 512 frames (the discoverer's) and of 256
  (max_hamming, min_hits)     the fraction of kernel pairs kept and the recall -- the share of the brute-force run's
                              matches (same six bounds) still found -- over a short grid
  TermDiscoverer.discover     wall time without and with the prefilter

Every GPU route settles the clock (untimed calls for 0.3 s) before its timed calls; medians are reported.
python tools/prefilter_time.py [--utts N] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from abnet3_amd import _lib
from abnet3_amd.prefilter import TermPrefilter, lsh_planes, lsh_signatures
from abnet3_amd.terms import TermDiscoverer, keep_matches, kernel_pairs
from tools.abx_time import median_ms, wall
from tools.terms_time import synthetic

HBM_PEAK, HBM_COPY = 8.0e12, 6.29e12


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--utts', type=int, default=64)
    ap.add_argument('--theta', type=float, default=0.25)
    ap.add_argument('--bits', type=int, default=64)
    ap.add_argument('--calls', type=int, default=7)
    ap.add_argument('--out', default=None)
    a = ap.parse_args()
    feats, times, planted = synthetic(a.utts)
    td = TermDiscoverer(feats, times, theta=a.theta)
    c = td.corpus
    rows, D = c.table.shape
    lib, ptr = _lib.load(), _lib.ptr
    dev = lambda x, dt: torch.from_numpy(np.ascontiguousarray(x, dtype=dt)).cuda()
    base = np.array([c.offset[k] for k in td.names], dtype=np.int64)
    length = np.array([c.length[k] for k in td.names], dtype=np.int32)
    n = len(td.names)
    upairs = [(u, v) for u in range(n) for v in range(u, n)]
    res = {'device': torch.cuda.get_device_name(0),
           'set': '%d utterances of 200-1000 frames (%d rows), D = %d; %d words of 50-90 frames planted %d times each with noise; '
                  'every utterance whole against every window of every utterance (itself included)' % (n, rows, D, len(planted), n // len(planted))}

    # --- signatures
    planes = dev(lsh_planes(D, a.bits, seed=0), np.float32)
    sig_out = {}
    big = torch.randn((1140000, D), device='cuda')
    for name, table in (('corpus_table', c.table), ('table_1140000_rows', big)):
        so = torch.empty((table.shape[0], a.bits // 32), dtype=torch.int32, device='cuda')
        lo_ = torch.empty(table.shape[0], dtype=torch.uint8, device='cuda')
        ms = median_ms(lambda: _lib.check(lib.abn_lsh_signatures(ptr(table), table.shape[0], D, ptr(planes), a.bits, ptr(so), ptr(lo_),
                                                                 _lib.stream()), 'abn_lsh_signatures'), a.calls)
        nbytes = table.numel() * 4
        sig_out[name] = {'rows': table.shape[0], 'D': D, 'bits': a.bits, 'table_bytes': nbytes, 'median_ms': round(ms, 4),
                         'table_bytes_per_s': round(nbytes / (ms * 1e-3), 1),
                         'fraction_of_hbm_peak_bound': round(nbytes / HBM_PEAK / (ms * 1e-3), 4),
                         'fraction_of_hbm_copy_bound': round(nbytes / HBM_COPY / (ms * 1e-3), 4),
                         'fp32_flops_per_s': round(2.0 * table.shape[0] * D * a.bits / (ms * 1e-3), 1)}
    del big, so, lo_
    res['abn_lsh_signatures'] = sig_out
    sig, live = lsh_signatures(c.table, planes)

    # --- the dot-plot kernel against the local alignment on the same pair table
    def pair_table(window):
        kp = np.array(kernel_pairs(length.tolist(), upairs, window), dtype=np.int64)
        o1, n1, o2, n2 = base[kp[:, 0]], length[kp[:, 0]], base[kp[:, 1]] + kp[:, 2], kp[:, 3].astype(np.int32)
        return ([dev(o1, np.int64), dev(n1, np.int32), dev(o2, np.int64), dev(n2, np.int32)], len(kp),
                int(np.dot(n1.astype(np.int64), n2.astype(np.int64))))

    def local(tab, P, o):
        _lib.check(lib.abn_dtw_local_batched(ptr(c.table), rows, ptr(c.table), rows, *[ptr(x) for x in tab], P, D,
                                             float(np.float32(a.theta)), 0, *[ptr(x) for x in o], _lib.stream()), 'abn_dtw_local_batched')

    def hits(tab, P, o, mh, span, dilate):
        _lib.check(lib.abn_lsh_diag_hits_batched(ptr(sig), ptr(live), rows, ptr(sig), ptr(live), rows, *[ptr(x) for x in tab], P,
                                                 sig.shape[1], mh, span, dilate, 0, *[ptr(x) for x in o], _lib.stream()),
                   'abn_lsh_diag_hits_batched')
    rate = lambda cells, ms: round(cells / (ms * 1e-3), 1)
    kern = {}
    for window in (512, 256):
        tab, P, cells = pair_table(window)
        lo = [torch.empty(P, dtype=torch.float64, device='cuda')] + [torch.empty(P, dtype=torch.int32, device='cuda') for _ in range(5)]
        ho = [torch.empty(P, dtype=torch.int32, device='cuda') for _ in range(3)]
        h_ms = median_ms(lambda: hits(tab, P, ho, a.bits // 4, 32, 1), a.calls)
        l_ms = median_ms(lambda: local(tab, P, lo), a.calls)
        h_ms2 = median_ms(lambda: hits(tab, P, ho, a.bits // 4, 32, 1), a.calls)
        l_ms2 = median_ms(lambda: local(tab, P, lo), a.calls)
        h0_ms = median_ms(lambda: hits(tab, P, ho, a.bits // 4, 32, 0), a.calls)
        h8_ms = median_ms(lambda: hits(tab, P, ho, a.bits // 4, 64, 8), a.calls)
        kern['window_%d' % window] = {
            'pairs': P, 'cells': cells,
            'abn_lsh_diag_hits_batched_ms': round(h_ms, 4), 'abn_lsh_diag_hits_batched_ms_again': round(h_ms2, 4),
            'abn_lsh_diag_hits_batched_cells_per_s': rate(cells, h_ms),
            'abn_dtw_local_batched_ms': round(l_ms, 4), 'abn_dtw_local_batched_ms_again': round(l_ms2, 4),
            'abn_dtw_local_batched_cells_per_s': rate(cells, l_ms),
            'diag_hits_over_local_cells_per_s': round(l_ms / h_ms, 2),
            'abn_lsh_diag_hits_batched_ms_dilate_0': round(h0_ms, 4), 'abn_lsh_diag_hits_batched_ms_span_64_dilate_8': round(h8_ms, 4)}
    res['kernels'] = dict(kern, settings='%d bits, max_hamming %d, span 32, dilate 1 unless named' % (a.bits, a.bits // 4))

    # --- kept pairs and recall over a short grid
    lengths = length.tolist()
    kp = kernel_pairs(lengths, upairs, td.window)
    brute = td.align(kp)
    key = lambda m: tuple(m)[:6]
    want = {key(m) for m in keep_matches(kp, brute, td.theta, td.min_frames, td.max_distance)}
    grid = []
    for mh in (4, 8, 12, 16, 20, 24):
        best = TermPrefilter(bits=a.bits, seed=0, max_hamming=mh, span=32, dilate=1).best_runs(td, kp)
        for min_hits in (16, 20, 24, 28, 32):
            mask = best >= min_hits
            sub = [q for q, m in zip(kp, mask) if m]
            got = {key(m) for m in keep_matches(sub, [r[mask] for r in brute], td.theta, td.min_frames, td.max_distance)}
            grid.append({'max_hamming': mh, 'min_hits': min_hits, 'kept_fraction': round(float(mask.mean()), 4),
                         'recall': round(len(got & want) / max(1, len(want)), 4)})
    res['grid'] = {'bits': a.bits, 'span': 32, 'dilate': 1, 'kernel_pairs': len(kp), 'brute_force_matches': len(want), 'rows': grid}

    # --- discover() end to end
    def timed(discoverer):
        m0, c0 = discoverer.discover()                                  # warm (with a prefilter: builds the signatures)
        walls = []
        for _ in range(3):
            w, (m, cl) = wall(discoverer.discover)
            walls.append(w)
            assert m == m0 and cl == c0
        return round(float(np.median(walls)), 4), m0, c0
    w_plain, m_plain, c_plain = timed(td)
    pre = TermPrefilter(bits=a.bits)
    w_pre, m_pre, c_pre = timed(TermDiscoverer(c, theta=a.theta, prefilter=pre))
    tdp = TermDiscoverer(c, theta=a.theta, prefilter=pre)
    tdp.discover()
    res['discover'] = {'without_prefilter_s_median': w_plain, 'matches': len(m_plain), 'clusters': len(c_plain),
                       'with_default_prefilter_s_median': w_pre, 'with_default_prefilter_matches': len(m_pre),
                       'with_default_prefilter_clusters': len(c_pre),
                       'with_default_prefilter_recall': round(len({key(m) for m in m_pre} & want) / max(1, len(want)), 4),
                       'default_prefilter': 'bits %d, max_hamming %d, span %d, dilate %d, min_hits %d (untuned)' % (
                           pre.bits, pre.max_hamming, pre.span, pre.dilate, pre.min_hits),
                       'kernel_pairs': tdp.n_kernel_pairs, 'aligned_pairs': tdp.n_aligned_pairs}
    res['protocol'] = ('settle 0.3 s of untimed calls, then the median of %d device-event timings per route; the routes alternate in '
                       'one process; abn_dtw_local_batched is the parent commit\'s machine code' % a.calls)
    print(json.dumps(res))
    if a.out:
        with open(a.out, 'w') as f:
            json.dump(res, f, indent=1)
            f.write('\n')


if __name__ == '__main__':
    main()
