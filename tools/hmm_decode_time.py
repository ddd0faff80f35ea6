"""Times the Viterbi decoding of the sticky HMM (abn_hmm_viterbi, abnet3_amd/csrc/hmm.hip).

Workloads and protocol: tools/hmm_time.py's (1.14 M frames as a synthetic clustered table, D = 40 with K = 256 and
K = 1024, D = 100 with K = 1024, the same seeded utterances of 200 .. 1000 frames and the same mixture of three EM
iterations); every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls (device events); medians,
minima and maxima.  Per workload, in the same process:

  abn_hmm_viterbi            one launch for the corpus, against
    abn_gmm_posteriors         its floor: the score GEMM, the exp and the store of a [T][K] table alone,
    abn_hmm_forward_backward   mode 1 (filter): its sum-product twin, one forward sweep,
    abn_kmeans_viterbi         its max-product twin at the same (D, K): centroids of three Lloyd iterations, penalty 6,
    torch route                per chunk of utterances the scores as a padded [utterances, max_len, K] torch.mm output, a
                               loop over time of batched torch ops with the same fp32 recurrence and a gather traceback;
                               its ids are compared with the kernel's
  --parent-lib FILE          abn_hmm_viterbi, abn_hmm_forward_backward (mode 1) and abn_kmeans_viterbi of another build of
                             the library (the parent commit's) timed alternately with this build's, 4 medians each,
                             outputs compared bit for bit; the bound on each ratio is 1 + twice the spread of the other
                             build alternating with itself (hmm_fit_time.versus_parent)

python tools/hmm_decode_time.py [--frames 1140000] [--stay 0.9] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from hmm_fit_time import versus_parent
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_viterbi(xc, A, B, c0, lw, ls, lr, off, lens, utt_chunk):
    """The composition: ids [T] int64 by the module's recurrence in batched torch ops (no BAD frames here)."""
    import torch
    T, K = xc.shape[0], A.shape[0]
    ids = torch.full((T,), -1, dtype=torch.int64, device=xc.device)
    for u0 in range(0, len(lens), utt_chunk):
        o, n = off[u0:u0 + utt_chunk], lens[u0:u0 + utt_chunk]
        U, L = len(n), int(n.max())
        rows = (o[:, None] + torch.arange(L, device=xc.device)[None, :]).clamp_(max=T - 1)
        x = xc[rows.reshape(-1)]
        S = (torch.addmm(c0[None, :], x, A.t()) + torch.mm(x * x, B.t())).view(U, L, K)
        del x
        stay = torch.zeros((U, L, K), dtype=torch.bool, device=xc.device)
        jst = torch.zeros((U, L), dtype=torch.int64, device=xc.device)
        W = None
        for t in range(L):
            if W is None:
                Uv = S[:, 0] + lw[None, :]
            else:
                a = W + ls[None, :]
                st = a > lr[None, :]
                stay[:, t] = st
                Uv = S[:, t] + torch.where(st, a, lr[None, :])
            M, j = Uv.max(dim=1)
            jst[:, t] = j
            Wn = Uv - M[:, None]
            W = Wn if W is None else torch.where((n > t)[:, None], Wn, W)
        out = torch.zeros((U, L), dtype=torch.int64, device=xc.device)
        cur = jst.gather(1, (n - 1)[:, None]).squeeze(1)
        for t in range(L - 1, -1, -1):
            out[:, t] = cur
            if t:
                keep = stay[:, t].gather(1, cur[:, None]).squeeze(1) | (n <= t)
                cur = torch.where(keep, cur, jst[:, t - 1])
        valid = torch.arange(L, device=xc.device)[None, :] < n[:, None]
        ids[rows[valid]] = out[valid]
    return ids


def workload(T, D, K, a, parent):
    import torch
    from abnet3_amd import _lib, gmm, hmm, kmeans
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    lab = torch.randint(0, K, (T // 8 + 1,), device='cuda', generator=g).repeat_interleave(8)[:T]      # 80 ms "phones"
    table = (centres[lab] + 1.5 * torch.randn(T, D, device='cuda', generator=g) + 5.0).contiguous()
    model = gmm.GmmPosteriorgram(K, n_iter=3, tol=-np.inf).fit(table)
    h = hmm.StickyHmmPosteriorgram(model, a.stay)
    shift, A, B, c0, w = h.device_tables(table.device)
    c = model.device_tables(table.device)[3]
    lw, ls, lr = (torch.from_numpy(t).cuda() for t in hmm.viterbi_tables(model.weights_, h.stay_))
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    p = _lib.ptr
    n_utt, max_len = len(len_h), int(len_h.max())
    ws_bytes = int(lib.abn_hmm_viterbi_ws_bytes(n_utt, max_len, K, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    lp = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    rho = float(np.float32(a.stay))
    res = {'T': T, 'D': D, 'K': K, 'stay': rho, 'utterances': n_utt, 'max_len': max_len, 'workspace_bytes': ws_bytes,
           'score_matrix_bytes_never_formed': 4 * T * K}

    def vit(which=lib, out=ids):
        _lib.check(which.abn_hmm_viterbi(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(lw), p(ls), p(lr), K,
                                         p(out), p(lp), p(nsw), p(ng), p(ws), ws.numel(), _lib.stream()), 'abn_hmm_viterbi')

    # ---- the sum-product twin (filter) and the floor: both write a [T][K] table --------------------------------------------
    fws = torch.empty(int(lib.abn_hmm_ws_bytes(n_utt, max_len, K, D)), dtype=torch.uint8, device='cuda')
    post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
    ll, st = (torch.zeros(n_utt, dtype=torch.float64, device='cuda') for _ in range(2))
    fng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')

    def fb(which=lib, out=post):
        _lib.check(which.abn_hmm_forward_backward(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(w), K, rho, 1,
                                                  p(out), p(ll), p(st), p(fng), p(fws), fws.numel(), _lib.stream()),
                   'abn_hmm_forward_backward')

    plain = torch.empty((T, K), dtype=torch.float32, device='cuda')

    def floor():
        gmm.posteriors(table, shift, A, B, c, out=plain)

    # ---- the max-product twin: k-means centroids at the same (D, K) -----------------------------------------------------
    ktable, kshift, good = kmeans.prepare(table, 'euclidean')
    kst = kmeans.LloydState(kmeans.initial_centroids(ktable, kshift, good, K, 0), T, table.device)
    for _ in range(3):
        kmeans.lloyd_iteration(ktable, kshift, kst)
    kws = torch.empty(int(lib.abn_kmeans_viterbi_ws_bytes(n_utt, max_len, K, D)), dtype=torch.uint8, device='cuda')
    kids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    kobj = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    knsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    pen = float(np.float32(a.penalty / 2.0))

    def kvit(which=lib, out=kids):
        _lib.check(which.abn_kmeans_viterbi(p(ktable), T, D, p(off), p(lens), n_utt, p(kshift), p(kst.m), p(kst.b), K, pen, p(out),
                                            p(kobj), p(knsw), p(kws), kws.numel(), _lib.stream()), 'abn_kmeans_viterbi')

    vit(), fb(), floor(), kvit()
    res['abn_hmm_viterbi'] = median_ms(vit)
    res['abn_gmm_posteriors'] = median_ms(floor)
    res['abn_hmm_forward_backward_filter'] = median_ms(fb)
    res['abn_kmeans_viterbi'] = dict(median_ms(kvit), penalty=a.penalty)
    res['abn_hmm_viterbi_again'] = median_ms(vit)
    ms = res['abn_hmm_viterbi']['median_ms']
    res['time_over_floor'] = round(ms / res['abn_gmm_posteriors']['median_ms'], 3)
    res['time_over_filter'] = round(ms / res['abn_hmm_forward_backward_filter']['median_ms'], 3)
    res['time_over_abn_kmeans_viterbi'] = round(ms / res['abn_kmeans_viterbi']['median_ms'], 3)
    res['frames_per_s'] = round(T / (ms * 1e-3), 1)
    # the whole launch charged to the sequential steps of a workgroup's utterances (its score tiles included): per frame
    groups = min(n_utt, 256)
    res['us_per_frame_step_upper_bound'] = round(ms * 1e3 / (T / float(groups)), 3)

    if parent is not None:
        def same(fn, out, other, rest):
            """`out` and the per-utterance outputs `rest` of fn under both builds"""
            fn()
            torch.cuda.synchronize()
            mine = [t.clone() for t in rest]
            fn(parent, other)
            torch.cuda.synchronize()
            return torch.equal(out, other) and all(torch.equal(m, t) for m, t in zip(mine, rest))

        other = torch.zeros((T, K), dtype=torch.float32, device='cuda')
        res['abn_hmm_forward_backward_vs_parent_build'] = versus_parent(fb, lambda: fb(parent, other),
                                                                        lambda: same(fb, post, other, (ll, fng)))
        del other
        oids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
        res['abn_hmm_viterbi_vs_parent_build'] = versus_parent(vit, lambda: vit(parent, oids),
                                                               lambda: same(vit, ids, oids, (lp, nsw, ng)))
        res['abn_kmeans_viterbi_vs_parent_build'] = versus_parent(kvit, lambda: kvit(parent, oids),
                                                                  lambda: same(kvit, kids, oids, (kobj, knsw)))
        del oids
    del post, plain
    torch.cuda.empty_cache()

    # ---- the torch route -----------------------------------------------------------------------------------------------
    xc = table - shift
    off64, len64 = off, lens.to(torch.int64)
    hold = {}

    def t_route():
        hold['ids'] = torch_viterbi(xc, A, B, c0, lw, ls, lr, off64, len64, a.utt_chunk)

    res['torch_route'] = dict(median_ms(t_route, calls=a.torch_calls), calls=a.torch_calls, utterances_per_chunk=a.utt_chunk)
    res['speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / ms, 3)
    vit()
    torch.cuda.synchronize()
    differ = int((ids.to(torch.int64) != hold['ids']).sum())
    host_ids = ids.cpu().numpy()
    seqs = kmeans.unit_sequences({u: host_ids[o:o + n] for u, (o, n) in enumerate(zip(off_h, len_h))})
    res['agreement'] = {'ids_that_differ_from_the_torch_route': differ, 'switches': int(nsw.sum()), 'good_frames': int(ng.sum()),
                        'mean_log_prob_per_frame': float(lp.sum() / ng.sum()), 'mean_loglik_per_frame_filter': float(ll.sum() / fng.sum()),
                        'symbols': int(sum(len(v) for v in seqs.values())),
                        'bitrate_bits_per_s': round(kmeans.bitrate(seqs, T * 0.01), 2)}
    print('D = %d, K = %d: viterbi %.3f ms (floor %.3f, filter %.3f, kmeans viterbi %.3f, torch %.1f), %d ids differ from the torch route'
          % (D, K, ms, res['abn_gmm_posteriors']['median_ms'], res['abn_hmm_forward_backward_filter']['median_ms'],
             res['abn_kmeans_viterbi']['median_ms'], res['torch_route']['median_ms'], differ), file=sys.stderr, flush=True)
    del hold, xc
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--penalty', type=float, default=6.0, help='abn_kmeans_viterbi\'s penalty (units of the distortion)')
    ap.add_argument('--utt-chunk', type=int, default=256, help='utterances per padded score tensor of the torch route')
    ap.add_argument('--torch-calls', type=int, default=15)
    ap.add_argument('--parent-lib', default=None, metavar='FILE', help='the parent commit\'s libabnet3_hip.so')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_decode_time.json'))
    a = ap.parse_args()
    import torch
    from abnet3_amd import _lib
    parent = None
    if a.parent_lib:
        lib = _lib.load()
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ('abn_hmm_forward_backward', 'abn_hmm_viterbi', 'abn_kmeans_viterbi'):
            fn, own = getattr(parent, name), getattr(lib, name)
            fn.restype, fn.argtypes = own.restype, own.argtypes
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15,
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
