"""Times the sticky-HMM forward-backward (abn_hmm_forward_backward, abnet3_amd/csrc/hmm.hip).

Workloads: tools/units_time.py's three shapes (1.14 M frames as a synthetic clustered table, D = 40 with K = 256 and
K = 1024, D = 100 with K = 1024), the frames cut into the same seeded utterances of 200 .. 1000 frames; the mixture is
three EM iterations from the documented initialisation.  Timed, per workload, in the same process:

  abn_hmm_forward_backward   mode 0 (smoothed) and mode 1 (filtered), one launch for the corpus (device events)
  floor                      abn_gmm_posteriors writing the same [T][K] table: the score GEMM, the exp and the store alone
  torch route                per chunk of utterances the scores as padded [utterances, max_len, K] torch.mm output, then a
                             loop over time of batched torch ops with the same fp32 recursion, forward and backward; its
                             gamma is compared with the kernel's

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls (the torch route: --torch-calls);
medians, minima and maxima are reported, with the ratios to the floor, mode 0 over mode 1, and the workspace bytes.

python tools/hmm_time.py [--frames 1140000] [--stay 0.9] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_forward_backward(xc, A, B, c0, w, off, lens, rho, utt_chunk, out):
    """The composition: gamma into out [T, K] by the module's recursion in batched torch ops (no BAD frames here)."""
    import torch
    T, K = xc.shape[0], A.shape[0]
    omr = 1.0 - rho
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
            u = bt[:, t] * (w[None, :] if a is None else rho * a + omr * w[None, :])
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
                nb = rho * e + omr * (w[None, :] * e).sum(dim=1, keepdim=True)
                bhat = torch.where((n > t)[:, None], nb, bhat)
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
    h = hmm.StickyHmmPosteriorgram(model, a.stay)
    shift, A, B, c0, w = h.device_tables(table.device)
    c = model.device_tables(table.device)[3]
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    n_utt, max_len = len(len_h), int(len_h.max())
    ws_bytes = int(lib.abn_hmm_ws_bytes(n_utt, max_len, K, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
    ll = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    st = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    rho = float(np.float32(a.stay))
    res = {'T': T, 'D': D, 'K': K, 'stay': rho, 'utterances': n_utt, 'max_len': max_len, 'workspace_bytes': ws_bytes,
           'output_bytes': 4 * T * K}

    def fb(mode):
        _lib.check(lib.abn_hmm_forward_backward(_lib.ptr(table), T, D, _lib.ptr(off), _lib.ptr(lens), n_utt, _lib.ptr(shift), _lib.ptr(A),
                                                _lib.ptr(B), _lib.ptr(c0), _lib.ptr(w), K, rho, mode, _lib.ptr(post), _lib.ptr(ll),
                                                _lib.ptr(st), _lib.ptr(ng), _lib.ptr(ws), ws.numel(), _lib.stream()),
                   'abn_hmm_forward_backward')

    plain = torch.empty((T, K), dtype=torch.float32, device='cuda')

    def floor():
        gmm.posteriors(table, shift, A, B, c, out=plain)

    xc = table - shift
    off64, len64 = off, lens.to(torch.int64)
    other = torch.zeros((T, K), dtype=torch.float32, device='cuda')

    def t_route():
        torch_forward_backward(xc, A, B, c0, w, off64, len64, rho, a.utt_chunk, other)

    fb(0), floor()
    res['smoothed'] = median_ms(lambda: fb(0))
    res['filtered'] = median_ms(lambda: fb(1))
    res['abn_gmm_posteriors'] = median_ms(floor)
    res['smoothed_again'] = median_ms(lambda: fb(0))
    res['torch_route'] = dict(median_ms(t_route, calls=a.torch_calls), calls=a.torch_calls, utterances_per_chunk=a.utt_chunk)
    sm, fi, fl = (res[k]['median_ms'] for k in ('smoothed', 'filtered', 'abn_gmm_posteriors'))
    res['smoothed_over_floor'] = round(sm / fl, 3)
    res['filtered_over_floor'] = round(fi / fl, 3)
    res['smoothed_over_filtered'] = round(sm / fi, 3)
    res['speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / sm, 3)
    res['frames_per_s_smoothed'] = round(T / (sm * 1e-3), 1)
    fb(0)
    torch.cuda.synchronize()
    res['agreement'] = {'max_abs_gamma_difference_from_the_torch_route': float((post - other).abs().max()),
                        'mean_loglik_per_frame': float(ll.sum() / ng.sum()), 'expected_stay_share': float(st.sum() / (ng - 1).clamp(min=0).sum())}
    print('D = %d, K = %d: smoothed %.3f ms, filtered %.3f ms, floor %.3f ms' % (D, K, sm, fi, fl), file=sys.stderr, flush=True)
    del xc, other, plain, post
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--utt-chunk', type=int, default=256, help='utterances per padded score tensor of the torch route')
    ap.add_argument('--torch-calls', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15,
           'workloads': [workload(a.frames, 40, 256, a), workload(a.frames, 40, 1024, a), workload(a.frames, 100, 1024, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
