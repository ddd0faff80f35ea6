"""Times the full-transition HMM forward-backward (abny_hmm_dense_forward_backward, abnet3_amd/csrc/hmm_dense.hip).

Workloads: tools/hmm_time.py's corpus (1.14 M frames as a synthetic clustered table, cut into the same kind of seeded
utterances of 200 .. 1000 frames; the mixture is three EM iterations from the documented initialisation) at
(D, K) = (40, 64), (40, 128), (100, 128).  The transition matrix is the sticky matrix of the mixture's weights, so the
sticky kernel computes the same model.  Timed, per workload, in the same process:

  dense                       mode 0 with and without the statistics, and mode 1, one launch for the corpus (device events)
  sticky                      abn_hmm_forward_backward_stats on the same model, alternating with the dense kernel
  floor                       abn_gmm_posteriors writing the same [T][K] table: the score GEMM, the exp and the store alone
  torch route                 per chunk of utterances the scores as a padded [utterances, max_len, K] tensor, then a loop over
                              time of batched torch ops (the K x K products as torch.matmul) with the same fp32 recursion,
                              forward and backward; its gamma is compared with the kernel's
  one fit iteration           TransitionHmmPosteriorgram.fit(n_iter=1) end to end (wall clock, with its read-back)

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls (the torch route: --torch-calls, 3 by
default: a call is a hundred thousand launches); medians, minima and maxima are reported, with microseconds per frame
and sweep, the ratio to the sticky kernel, and the share of the device's fp32 FMA rate that the K^2 products of the two
sweeps reach (2 x 2 K^2 flop per frame against 256 CUs x 128 lanes x 2 flop x the clock).

python tools/hmm_dense_time.py [--frames 1140000] [--stay 0.9] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PEAK_FP32_FMA_FLOPS = 256 * 128 * 2 * 2.4e9      # vector fp32 FMA, no packed math, at the 2.4 GHz peak clock


def torch_forward_backward(xc, A, B, c0, init, trans, off, lens, utt_chunk, out):
    """The composition: gamma into out [T, K] by the module's recursion in batched torch ops (no BAD frames here)."""
    import torch
    T, K = xc.shape[0], A.shape[0]
    tt = trans.t().contiguous()
    for u0 in range(0, len(lens), utt_chunk):
        o, n = off[u0:u0 + utt_chunk], lens[u0:u0 + utt_chunk]
        U, L = len(n), int(n.max())
        rows = (o[:, None] + torch.arange(L, device=xc.device)[None, :]).clamp_(max=T - 1)
        x = xc[rows.reshape(-1)]
        S = (torch.addmm(c0[None, :], x, A.t()) + torch.mm(x * x, B.t())).view(U, L, K)
        bt = torch.exp(S - S.max(dim=2, keepdim=True).values)
        del S
        ahat = torch.empty_like(bt)
        c = torch.empty((U, L), dtype=torch.float32, device=xc.device)
        a = None
        for t in range(L):
            u = bt[:, t] * (init[None, :] if a is None else torch.matmul(a, trans))
            ct = u.sum(dim=1)
            an = u / ct[:, None]
            a = an if a is None else torch.where((n > t)[:, None], an, a)
            ahat[:, t] = a
            c[:, t] = ct
        bhat = torch.ones((U, K), dtype=torch.float32, device=xc.device)
        for t in range(L - 1, -1, -1):
            ahat[:, t] *= bhat
            if t:
                e = bt[:, t] * bhat / c[:, t][:, None]
                bhat = torch.where((n > t)[:, None], torch.matmul(e, tt), bhat)
        valid = torch.arange(L, device=xc.device)[None, :] < n[:, None]
        out[rows[valid]] = ahat[valid]
    return out


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
    sticky = hmm.StickyHmmPosteriorgram(model, a.stay)
    shift, A, B, c0, wd = sticky.device_tables(table.device)
    c = model.device_tables(table.device)[3]
    init_h, trans_h = hmm.sticky_transitions(model.weights_, a.stay)
    init, trans = torch.from_numpy(init_h).cuda(), torch.from_numpy(trans_h).cuda()
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    n_utt, max_len = len(len_h), int(len_h.max())
    ws_bytes = int(lib.abny_hmm_dense_ws_bytes(n_utt, max_len, K, D))
    ws = torch.empty(max(ws_bytes, int(lib.abn_hmm_ws_bytes(n_utt, max_len, K, D))), dtype=torch.uint8, device='cuda')
    post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
    ll = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    st = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    sk = torch.zeros((n_utt, K), dtype=torch.float64, device='cuda')
    stats = torch.zeros((K + 1, K), dtype=torch.float64, device='cuda')
    rho = float(np.float32(a.stay))
    res = {'T': T, 'D': D, 'K': K, 'stay': rho, 'utterances': n_utt, 'max_len': max_len, 'workspace_bytes': ws_bytes,
           'output_bytes': 4 * T * K}
    p = _lib.ptr

    def dense(mode, with_stats):
        _lib.check(lib.abny_hmm_dense_forward_backward(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(init),
                                                       p(trans), K, mode, p(post), p(ll), p(ng), p(stats if with_stats else None),
                                                       p(ws), ws.numel(), _lib.stream()), 'abny_hmm_dense_forward_backward')

    def sticky_fb():
        _lib.check(lib.abn_hmm_forward_backward_stats(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(wd), K, rho,
                                                      0, p(post), p(ll), p(st), p(ng), p(sk), p(ws), ws.numel(), _lib.stream()),
                   'abn_hmm_forward_backward_stats')

    plain = torch.empty((T, K), dtype=torch.float32, device='cuda')

    def floor():
        gmm.posteriors(table, shift, A, B, c, out=plain)

    xc = table - shift
    off64, len64 = off, lens.to(torch.int64)
    other = torch.zeros((T, K), dtype=torch.float32, device='cuda')

    def t_route():
        torch_forward_backward(xc, A, B, c0, init, trans, off64, len64, a.utt_chunk, other)

    dense(0, True), sticky_fb(), floor()
    res['dense_smoothed_stats'] = median_ms(lambda: dense(0, True))
    res['sticky_smoothed_stats'] = median_ms(sticky_fb)
    res['dense_smoothed'] = median_ms(lambda: dense(0, False))
    res['dense_filtered'] = median_ms(lambda: dense(1, False))
    res['abn_gmm_posteriors'] = median_ms(floor)
    res['dense_smoothed_stats_again'] = median_ms(lambda: dense(0, True))
    res['sticky_smoothed_stats_again'] = median_ms(sticky_fb)
    res['torch_route'] = dict(median_ms(t_route, calls=a.torch_calls), calls=a.torch_calls, utterances_per_chunk=a.utt_chunk)
    ds, dp, df, sy, fl = (res[k]['median_ms'] for k in ('dense_smoothed_stats', 'dense_smoothed', 'dense_filtered',
                                                        'sticky_smoothed_stats', 'abn_gmm_posteriors'))
    res['dense_over_sticky'] = round(ds / sy, 3)
    res['dense_over_floor'] = round(ds / fl, 3)
    res['stats_over_no_stats'] = round(ds / dp, 3)
    res['speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / dp, 3)
    res['us_per_frame_and_sweep'] = round(dp * 1e3 / (2.0 * T), 6)
    res['us_per_frame_and_sweep_of_a_workgroup'] = round(dp * 1e3 / (2.0 * T) * min(n_utt, 256), 4)
    res['share_of_fp32_fma_rate'] = round(2.0 * 2.0 * K * K * T / (dp * 1e-3) / PEAK_FP32_FMA_FLOPS, 5)
    dense(0, True)
    torch.cuda.synchronize()
    xi_diag = torch.diagonal(stats[:K]).clone()
    agreement = {'max_abs_gamma_difference_from_the_torch_route': float((post - other).abs().max()),
                 'mean_loglik_per_frame': float(ll.sum() / ng.sum()), 'sum_xi_over_transitions': float(stats[:K].sum() / (ng - 1).clamp(min=0).sum())}
    sticky_fb()
    torch.cuda.synchronize()
    stay_k = xi_diag * rho / (rho + (1.0 - rho) * wd.to(torch.float64))
    agreement['max_abs_stay_k_difference_from_the_sticky_kernel'] = float((stay_k - sk.sum(dim=0)).abs().max())
    res['agreement'] = agreement
    from abnet3_amd.dataloader import DeviceCorpus
    names = ['u%05d' % i for i in range(n_utt)]
    corpus = DeviceCorpus.from_table(table, names, len_h.tolist(), {k: np.zeros(0) for k in names})
    hmm.TransitionHmmPosteriorgram(model, trans_h, init_h).fit(corpus, n_iter=1)      # (the first call's allocations)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    hmm.TransitionHmmPosteriorgram(model, trans_h, init_h).fit(corpus, n_iter=1)
    torch.cuda.synchronize()
    res['one_fit_iteration_ms'] = round((time.perf_counter() - t0) * 1e3, 3)
    print('D = %d, K = %d: dense %.3f ms (%.3f without statistics, %.3f filtered), sticky %.3f ms, floor %.3f ms, torch %.1f ms'
          % (D, K, ds, dp, df, sy, fl, res['torch_route']['median_ms']), file=sys.stderr, flush=True)
    del xc, other, plain, post
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--utt-chunk', type=int, default=256, help='utterances per padded score tensor of the torch route')
    ap.add_argument('--torch-calls', type=int, default=3)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_dense_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15,
           'workloads': [workload(a.frames, 40, 64, a), workload(a.frames, 40, 128, a), workload(a.frames, 100, 128, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
