"""Times the Baum-Welch step of the sticky HMM (abn_hmm_forward_backward_stats and abn_hmm_accumulate,
abnet3_amd/csrc/hmm.hip) and StickyHmmPosteriorgram.fit.

Workloads and protocol: tools/hmm_time.py's (1.14 M frames, D = 40 with K = 256 and K = 1024, D = 100 with K = 1024, the
same seeded utterances and mixture); every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls
(device events); medians, minima and maxima.  Per workload, in the same process:

  abn_hmm_accumulate         on the smoothed gamma table, against
    abn_gmm_accumulate         at the same shape (it recomputes its responsibilities from the scores: no table is read),
    torch route                torch.mm(post.t(), [xc | xc^2 | 1]) on the same tables (the augmented table built once, untimed),
    HBM floor                  the time 4 T K bytes take at the HBM peak (8 TB/s)
  stats entry                abn_hmm_forward_backward_stats against abn_hmm_forward_backward (mode 0), alternating
  fit iteration              one iteration of StickyHmmPosteriorgram.fit, read-back and host M-step included (wall clock),
                             against the forward-backward launch alone
  --parent-lib FILE          abn_hmm_forward_backward (mode 0) and abn_hmm_forward_backward_stats of another build of the
                             library (the parent commit's) timed alternately with this build's, `repeats` medians each,
                             outputs compared bit for bit; the other build alternating with itself gives the spread, and
                             the bound on the ratio is 1 + twice that spread

python tools/hmm_fit_time.py [--frames 1140000] [--stay 0.9] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HBM_PEAK = 8.0e12


def alternate(this_fn, other_fn, repeats=4):
    """Medians of the two routes, alternating, `repeats` times each: the ratio of the medians of the medians and the
    second route's relative spread (max - min) / median over its repeats."""
    a, b = [], []
    for _ in range(repeats):
        a.append(median_ms(this_fn)['median_ms'])
        b.append(median_ms(other_fn)['median_ms'])
    spread = (max(b) - min(b)) / float(np.median(b))
    return {'first_ms': a, 'second_ms': b, 'ratio_of_medians': round(float(np.median(a) / np.median(b)), 4),
            'second_relative_spread': round(spread, 4)}


def versus_parent(this_fn, parent_fn, same):
    """This build against the parent build, alternating, and the parent build against itself the same way: its spread is
    (max - min) / median over the 2 x `repeats` medians of that second run, the bound on the ratio 1 + twice the spread.
    same(): whether the two builds' outputs are bit-identical (it runs both once more)."""
    blk = alternate(this_fn, parent_fn)
    own = alternate(parent_fn, parent_fn)
    ms = own['first_ms'] + own['second_ms']
    spread = (max(ms) - min(ms)) / float(np.median(ms))
    blk.update(first='this build', second='parent build', parent_against_itself_ms=ms, parent_spread=round(spread, 4),
               bound=round(1.0 + 2.0 * spread, 4), outputs_bit_identical=bool(same()))
    blk['within_the_bound'] = bool(blk['ratio_of_medians'] <= blk['bound'])
    return blk


def workload(T, D, K, a, parent):
    import torch
    from abnet3_amd import _lib, gmm, hmm
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    lab = torch.randint(0, K, (T // 8 + 1,), device='cuda', generator=g).repeat_interleave(8)[:T]      # 80 ms "phones"
    table = (centres[lab] + 1.5 * torch.randn(T, D, device='cuda', generator=g) + 5.0).contiguous()
    model = gmm.GmmPosteriorgram(K, n_iter=3, tol=-np.inf).fit(table)
    h = hmm.StickyHmmPosteriorgram(model, a.stay)
    shift, A, B, c0, w = h.device_tables(table.device)
    c = model.device_tables(table.device)[3]
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    n_utt, max_len = len(len_h), int(len_h.max())
    ws = torch.empty(int(lib.abn_hmm_ws_bytes(n_utt, max_len, K, D)), dtype=torch.uint8, device='cuda')
    post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
    ll, st = (torch.zeros(n_utt, dtype=torch.float64, device='cuda') for _ in range(2))
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    sk = torch.zeros((n_utt, K), dtype=torch.float64, device='cuda')
    rho = float(np.float32(a.stay))
    res = {'T': T, 'D': D, 'K': K, 'stay': rho, 'utterances': n_utt, 'max_len': max_len, 'post_bytes': 4 * T * K}
    p = _lib.ptr
    head = lambda out: [p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(w), K, rho, 0, p(out), p(ll), p(st), p(ng)]
    tail = [p(ws), ws.numel(), _lib.stream()]

    def fb(which=lib, out=post):
        _lib.check(which.abn_hmm_forward_backward(*(head(out) + tail)), 'abn_hmm_forward_backward')

    def fb_stats(which=lib, out=post):
        _lib.check(which.abn_hmm_forward_backward_stats(*(head(out) + [p(sk)] + tail)), 'abn_hmm_forward_backward_stats')

    # ---- the stats entry against the plain one ------------------------------------------------------------------------
    fb(), fb_stats()
    res['stats_entry_vs_plain'] = dict(alternate(fb_stats, fb), first='abn_hmm_forward_backward_stats', second='abn_hmm_forward_backward')
    if parent is not None:
        other = torch.zeros((T, K), dtype=torch.float32, device='cuda')

        def same(fn):
            """post, loglik, stays, n_good and stay_k of fn under both builds"""
            sk.zero_()
            fn()
            torch.cuda.synchronize()
            mine = [t.clone() for t in (ll, st, ng, sk)]
            sk.zero_()
            fn(parent, other)
            torch.cuda.synchronize()
            return torch.equal(post, other) and all(torch.equal(m, t) for m, t in zip(mine, (ll, st, ng, sk)))

        res['abn_hmm_forward_backward_vs_parent_build'] = versus_parent(fb, lambda: fb(parent, other), lambda: same(fb))
        res['abn_hmm_forward_backward_stats_vs_parent_build'] = versus_parent(fb_stats, lambda: fb_stats(parent, other),
                                                                              lambda: same(fb_stats))
        del other

    # ---- abn_hmm_accumulate -------------------------------------------------------------------------------------------
    fb_stats()
    aws = torch.empty(int(lib.abn_hmm_accumulate_ws_bytes(T, K, D, 0)), dtype=torch.uint8, device='cuda')
    sums = torch.zeros((K, 2 * D + 1), dtype=torch.float64, device='cuda')

    def acc():
        _lib.check(lib.abn_hmm_accumulate(p(table), T, D, p(shift), p(post), K, 0, p(sums), p(aws), aws.numel(), _lib.stream()),
                   'abn_hmm_accumulate')

    lse, _ = gmm.posteriors(table, shift, A, B, c, want_post=False)
    gws = torch.empty(int(lib.abn_gmm_ws_bytes(T, K, D, 0)), dtype=torch.uint8, device='cuda')

    def gacc():
        _lib.check(lib.abn_gmm_accumulate(p(table), T, D, p(shift), p(A), p(B), p(c), K, p(lse), 0, p(gws), gws.numel(), _lib.stream()),
                   'abn_gmm_accumulate')

    xc = table - shift
    aug = torch.cat([xc, xc * xc, torch.ones((T, 1), dtype=torch.float32, device='cuda')], dim=1).contiguous()
    del xc
    tsum = [None]

    def tmm():
        tsum[0] = torch.mm(post.t(), aug)

    acc(), gacc(), tmm()
    res['abn_hmm_accumulate'] = median_ms(acc)
    res['abn_gmm_accumulate'] = median_ms(gacc)
    res['torch_mm'] = median_ms(tmm)
    res['abn_hmm_accumulate_again'] = median_ms(acc)
    am = res['abn_hmm_accumulate']['median_ms']
    res['hbm_floor_ms'] = round(4.0 * T * K / HBM_PEAK * 1e3, 3)
    res['accumulate_over_hbm_floor'] = round(am / res['hbm_floor_ms'], 3)
    res['accumulate_over_abn_gmm_accumulate'] = round(am / res['abn_gmm_accumulate']['median_ms'], 3)
    res['speedup_over_torch_mm'] = round(res['torch_mm']['median_ms'] / am, 3)
    res['read_rate_TB_per_s'] = round(4.0 * T * K / (am * 1e-3) / 1e12, 3)
    acc(), tmm()
    torch.cuda.synchronize()
    res['agreement'] = {'max_rel_difference_from_torch_mm': float(((sums - tsum[0].to(torch.float64)).abs().max() / sums.abs().max()).item())}
    del aug, tsum

    # ---- one iteration of fit against the forward-backward alone --------------------------------------------------------
    offs, lens_h = off_h, len_h.astype(np.int64)
    feats = None
    from abnet3_amd.dataloader import DeviceCorpus
    names = ['u%05d' % i for i in range(n_utt)]
    if int(offs[-1] + lens_h[-1]) == T and (offs == np.cumsum(lens_h) - lens_h).all():
        feats = DeviceCorpus.from_table(table, names, [int(n) for n in lens_h], {k: None for k in names})
    del post, sk
    torch.cuda.empty_cache()
    if feats is not None:
        walls = []
        hh = hmm.StickyHmmPosteriorgram(model, a.stay)
        hh.fit(feats, n_iter=1, tol=-np.inf)                                 # warm
        for n_iter in (1, 3):
            ts = []
            for _ in range(5):
                hh = hmm.StickyHmmPosteriorgram(model, a.stay)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hh.fit(feats, n_iter=n_iter, tol=-np.inf)
                torch.cuda.synchronize()
                ts.append(time.perf_counter() - t0)
            walls.append(float(np.median(ts)))
        per_iter = (walls[1] - walls[0]) / 2.0 * 1e3                         # (the scratch table's allocation cancels)
        fbm = float(np.median(res['stats_entry_vs_plain']['second_ms']))
        res['fit'] = {'one_iteration_s': round(walls[0], 4), 'three_iterations_s': round(walls[1], 4), 'ms_per_further_iteration': round(per_iter, 3),
                      'iteration_over_forward_backward': round(per_iter / fbm, 3), 'log_likelihoods': hh.log_likelihoods, 'stay': hh.stay_}
    print('D = %d, K = %d: accumulate %.3f ms (gmm %.3f, torch.mm %.3f, HBM floor %.3f), stats / plain %.4f'
          % (D, K, am, res['abn_gmm_accumulate']['median_ms'], res['torch_mm']['median_ms'], res['hbm_floor_ms'],
             res['stats_entry_vs_plain']['ratio_of_medians']), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--parent-lib', default=None, metavar='FILE', help='the parent commit\'s libabnet3_hip.so')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_fit_time.json'))
    a = ap.parse_args()
    import torch
    from abnet3_amd import _lib
    parent = None
    if a.parent_lib:
        lib = _lib.load()
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ('abn_hmm_forward_backward', 'abn_hmm_forward_backward_stats'):
            fn, own = getattr(parent, name), getattr(lib, name)
            fn.restype, fn.argtypes = own.restype, own.argtypes
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'hbm_peak_bytes_per_s': HBM_PEAK,
           'protocol': 'settle 0.3 s of untimed calls, then the median of 15 device-event timings per route; alternating routes '
                       'take 4 medians each in one process',
           'workloads': [workload(a.frames, 40, 256, a, parent), workload(a.frames, 40, 1024, a, parent),
                         workload(a.frames, 100, 1024, a, parent)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
