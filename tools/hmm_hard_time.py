"""Times the hard statistics of the full-transition HMM's Viterbi training (abnv_hmm_hard_stats, abnet3_amd/csrc/hmm_hard.hip)
and one iteration of TransitionHmmPosteriorgram.fit_viterbi.

Workloads: tools/hmm_dense_decode_time.py's corpus (1.14 M frames as a synthetic clustered table, cut into the same kind of
seeded utterances of 200 .. 1000 frames; the mixture is three EM iterations from the documented initialisation; the
transition matrix is the sticky matrix of the mixture's weights at stay 0.9) at (D, K) = (40, 64), (40, 128).  The ids are the
corpus' own best path (abnz_hmm_dense_viterbi).  Timed, per workload, in the same process and alternating (device events):

  hard stats        abnv_hmm_hard_stats, min_duration 1 and 3 (two memsets and three launches)
  kmeans pass       abn_kmeans_accumulate + abn_kmeans_update (statistics only) on the same rows and ids: the nearest existing
                    pass and a floor, not a competitor -- it forms S1 and the distortion, no S2 and no transition counts
  torch route       index_add_ for S1 / S2 / N and bincount of prev * K + cur for the bigrams, on the same tensors

and, end to end with the host's share (wall clock around a synchronised call): one fit_viterbi iteration at min_duration 1
and 3 and one Baum-Welch ``fit`` iteration.  Every route settles the clock (untimed calls for 0.3 s) before its 15 timed
calls; medians, minima and maxima are reported, with the share of the byte bound T (4 D + 4) at 6.3 TB/s.

Before anything is timed the entry runs on exact inputs (integer frames, an integer shift: every fp32 sum exact) laid out as
the timed corpus' first utterances, and counts, sums and n_good must equal tests/hmm_hard_np.py's; otherwise the run reports
failure and exits 1.

python tools/hmm_hard_time.py [--frames 1140000] [--stay 0.9] [--check-utterances 6] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms, settle
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
HBM_BYTES_PER_S = 6.3e12


def exact_check(off_h, len_h, n_check, D, K):
    """The entry against the restatement on exact inputs laid out as the corpus' first n_check utterances, S = 1 and 3."""
    import torch
    import hmm_hard_np as hh
    from abnet3_amd import hmm
    off, lens = off_h[:n_check], len_h[:n_check]
    T = int((off + lens).max())
    rng = np.random.default_rng(K)
    x = rng.integers(-8, 9, size=(T, D)).astype(np.float32)
    shift = rng.integers(-2, 3, size=D).astype(np.float32)
    ids = np.repeat(rng.integers(-1, K, size=T // 3 + 1), 3)[:T].astype(np.int32)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    same = []
    for S in (1, 3):
        got = hmm.hard_stats(dev(x), off, lens, dev(shift), dev(ids), K, min_duration=S)
        torch.cuda.synchronize()
        ref = hh.hard_stats(x, off, lens, shift, ids, K, S)
        same += [bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(got, ref)]
    return {'ok': all(same), 'utterances': int(n_check), 'frames': int(lens.sum()), 'counts_sums_n_good_equal_at_1_and_3': same}


def wall_ms(fn, calls=15):
    """median_ms with the host's share: wall clock around a synchronised call."""
    import torch
    settle(fn)
    ts = []
    for _ in range(calls):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(float(min(ts)), 3), 'max_ms': round(float(max(ts)), 3)}


def workload(T, D, K, a):
    import torch
    from abnet3_amd import _lib, gmm, hmm
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    lab = torch.randint(0, K, (T // 8 + 1,), device='cuda', generator=g).repeat_interleave(8)[:T]      # 80 ms "phones"
    table = (centres[lab] + 1.5 * torch.randn(T, D, device='cuda', generator=g) + 5.0).contiguous()
    model = gmm.GmmPosteriorgram(K, n_iter=3, tol=-np.inf).fit(table)
    w = np.maximum(model.weights_, 1e-8)
    model.weights_ = w / w.sum()
    off_h, len_h = cut(T, D + K)
    res = {'T': T, 'D': D, 'K': K, 'stay': float(np.float32(a.stay)), 'utterances': len(len_h), 'max_len': int(len_h.max())}
    res['exact_check'] = exact_check(off_h, len_h, a.check_utterances, D, K)
    if not res['exact_check']['ok']:
        return res
    init_h, trans_h = hmm.sticky_transitions(model.weights_, a.stay)
    h = hmm.TransitionHmmPosteriorgram(model, trans_h, init_h)
    shift, A, B, c0, _, _ = h.device_tables(table.device)
    li, lt = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in hmm.log_transitions(init_h, trans_h))
    ids = hmm.dense_viterbi(table, off_h, len_h, shift, A, B, c0, li, lt)[0]
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib, p = _lib.load(), _lib.ptr
    n_utt = len(len_h)
    sizes = {'hard_stats': int(lib.abnv_hmm_hard_stats_ws_bytes(T, n_utt, K, D, 0)), 'kmeans_pass': int(lib.abn_kmeans_ws_bytes(T, K, D, 0))}
    res['workspace_bytes'] = sizes
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device='cuda')
    counts = torch.empty((K + 1, K), dtype=torch.int64, device='cuda')
    sums = torch.empty((K, 2 * D + 1), dtype=torch.float64, device='cuda')
    ng = torch.empty(n_utt, dtype=torch.int32, device='cuda')
    km_sums = torch.empty((K, D + 1), dtype=torch.float64, device='cuda')
    km_stats = torch.empty(4, dtype=torch.float64, device='cuda')
    means32 = torch.from_numpy(np.ascontiguousarray((model.means_ - model.shift_.astype(np.float64)).astype(np.float32))).cuda()

    def hard(S):
        def call():
            _lib.check(lib.abnv_hmm_hard_stats(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(ids), K, S, 0, p(counts), p(sums), p(ng),
                                               p(ws), sizes['hard_stats'], _lib.stream()), 'abnv_hmm_hard_stats')
        return call

    def kmeans_pass():
        _lib.check(lib.abn_kmeans_accumulate(p(table), T, D, p(shift), p(means32), K, p(ids), 0, p(ws), sizes['kmeans_pass'], _lib.stream()),
                   'abn_kmeans_accumulate')
        _lib.check(lib.abn_kmeans_update(p(ws), sizes['kmeans_pass'], p(ids), T, K, D, 0, 0, p(km_sums), p(None), p(None), p(None),
                                         p(km_stats), _lib.stream()), 'abn_kmeans_update')

    inner = torch.ones(T, dtype=torch.bool, device='cuda')          # a frame with a predecessor in its own utterance
    inner[off] = False
    torch_out = {}

    def torch_route():
        i64 = ids.to(torch.int64)
        xc = table - shift
        torch_out['S1'] = torch.zeros((K, D), dtype=torch.float32, device='cuda').index_add_(0, i64, xc)
        torch_out['S2'] = torch.zeros((K, D), dtype=torch.float32, device='cuda').index_add_(0, i64, xc * xc)
        torch_out['N'] = torch.bincount(i64, minlength=K)
        pair = (i64[:-1] * K + i64[1:])[inner[1:]]
        torch_out['bigrams'] = torch.bincount(pair, minlength=K * K).view(K, K)

    hard(1)(), kmeans_pass(), torch_route()
    torch.cuda.synchronize()
    # (the corpus has no BAD frame, so the torch route counts what the entry counts at min_duration 1)
    hard(1)()
    torch.cuda.synchronize()
    res['torch_route_agrees'] = {'bigrams_equal': bool(torch.equal(torch_out['bigrams'], counts[:K])),
                                 'N_equal': bool(torch.equal(torch_out['N'].to(torch.float64), sums[:, 2 * D])),
                                 'largest_relative_S1_S2_difference': float(
                                     ((torch.cat([torch_out['S1'], torch_out['S2']], dim=1).to(torch.float64) - sums[:, :2 * D]).abs() /
                                      sums[:, :2 * D].abs().clamp(min=1.0)).max())}
    res['hard_stats'] = median_ms(hard(1))
    res['kmeans_pass'] = median_ms(kmeans_pass)
    res['torch_route'] = median_ms(torch_route)
    res['hard_stats_min_duration_3'] = median_ms(hard(3))
    res['hard_stats_again'] = median_ms(hard(1))
    res['kmeans_pass_again'] = median_ms(kmeans_pass)
    hs, km, tr = (res[k]['median_ms'] for k in ('hard_stats', 'kmeans_pass', 'torch_route'))
    moved = T * (4.0 * D + 4.0)
    res['byte_bound'] = {'bytes': moved, 'hbm_bytes_per_s': HBM_BYTES_PER_S, 'bound_ms': round(moved / HBM_BYTES_PER_S * 1e3, 4),
                         'share_of_the_bound_reached': round(moved / (hs * 1e-3) / HBM_BYTES_PER_S, 4)}
    res['hard_stats_over_kmeans_pass'] = round(hs / km, 3)
    res['hard_stats_over_torch_route'] = round(hs / tr, 3)
    del torch_out, inner
    # one training iteration end to end, host included; every call starts from the same parameters
    from abnet3_amd.dataloader import DeviceCorpus
    names = ['u%05d' % i for i in range(n_utt)]
    corpus = DeviceCorpus.from_table(table, names, [int(n) for n in len_h], {k: np.zeros(0) for k in names})

    def fit_viterbi(S):
        def call():
            hmm.TransitionHmmPosteriorgram(model, trans_h, init_h).fit_viterbi(corpus, n_iter=1, min_duration=S)
        return call

    def fit_bw():
        hmm.TransitionHmmPosteriorgram(model, trans_h, init_h).fit(corpus, n_iter=1)

    fit_viterbi(1)(), fit_bw()
    res['fit_viterbi_iteration'] = wall_ms(fit_viterbi(1))
    res['fit_iteration'] = wall_ms(fit_bw)
    res['fit_viterbi_iteration_min_duration_3'] = wall_ms(fit_viterbi(3))
    res['fit_viterbi_iteration_again'] = wall_ms(fit_viterbi(1))
    fv, fb, f3 = (res[k]['median_ms'] for k in ('fit_viterbi_iteration', 'fit_iteration', 'fit_viterbi_iteration_min_duration_3'))
    res['fit_viterbi_over_fit'] = round(fv / fb, 3)
    res['fit_viterbi_min_duration_3_over_1'] = round(f3 / fv, 3)
    print('D = %d, K = %d: hard stats %.3f ms, kmeans pass %.3f ms, torch route %.3f ms; fit_viterbi iteration %.2f ms (S = 3: %.2f), fit '
          'iteration %.2f ms' % (D, K, hs, km, tr, fv, f3, fb), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--check-utterances', type=int, default=6)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_hard_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'workloads': []}
    for D, K in ((40, 64), (40, 128)):
        res['workloads'].append(workload(a.frames, D, K, a))
        if not res['workloads'][-1]['exact_check']['ok']:
            res['failed'] = 'the entry differs from tests/hmm_hard_np.py on exact inputs (D = %d, K = %d)' % (D, K)
            break
    print(json.dumps(res))
    if 'failed' in res:
        print('FAILED: ' + res['failed'], file=sys.stderr)
        return 1
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    return 0


if __name__ == '__main__':
    sys.exit(main())
