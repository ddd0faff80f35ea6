"""Times the penalised unit segmentation (abn_kmeans_viterbi, abnet3_amd/csrc/kmeans.hip).

Workloads: tools/kmeans_time.py's three shapes (1.14 M frames as a synthetic clustered table, D = 40 with K = 256 and
K = 1024, D = 100 with K = 1024), the frames cut into seeded utterances of 200 .. 1000 frames.  Timed, per workload, in
the same process, alternating:

  abn_kmeans_viterbi   one launch for the corpus (device events)
  floor (a)            abn_kmeans_assign on the same table: the score GEMM alone
  torch route (b)      what existed before: per chunk of utterances a torch.mm into padded [utterances, max_len, K] scores,
                       a loop over time of batched torch ops with the same fp32 recurrence, and a gather traceback; its ids
                       are compared with the kernel's (they may differ where torch's GEMM rounds a near-tie the other way,
                       and torch.max does not promise the lowest index on exact ties)

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls (the torch route: --torch-calls);
medians, minima and maxima are reported, with cells/s (T x K per second), the share of the fp32 matrix-core roof that
the score part 2 T K (D + 1) flop would take of the kernel's time, the workspace bytes, and bitrate / switch count at a
few penalties.

python tools/units_time.py [--frames 1140000] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import FP32_MFMA_FLOPS, median_ms

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAME_SECONDS = 0.01


def cut(T, seed):
    """Seeded utterance lengths of 200 .. 1000 frames that tile T rows (the last one takes what is left)."""
    rng = np.random.default_rng(seed)
    lens = []
    left = T
    while left > 0:
        n = int(min(left, rng.integers(200, 1001)))
        lens.append(n)
        left -= n
    lens = np.array(lens, dtype=np.int64)
    return np.cumsum(lens) - lens, lens


def torch_viterbi(xc, m, b, off, lens, p, utt_chunk):
    """The composition: ids [T] int64 by the module's recurrence in batched torch ops."""
    import torch
    T, K = xc.shape[0], m.shape[0]
    ids = torch.full((T,), -1, dtype=torch.int64, device=xc.device)
    neg_p = torch.tensor(-p, dtype=torch.float32, device=xc.device)
    for u0 in range(0, len(lens), utt_chunk):
        o, n = off[u0:u0 + utt_chunk], lens[u0:u0 + utt_chunk]
        U, L = len(n), int(n.max())
        rows = (o[:, None] + torch.arange(L, device=xc.device)[None, :]).clamp_(max=T - 1)
        S = torch.addmm(b[None, :], xc[rows.reshape(-1)], m.t()).view(U, L, K)
        stay = torch.zeros((U, L, K), dtype=torch.bool, device=xc.device)
        jst = torch.zeros((U, L), dtype=torch.int64, device=xc.device)
        W = None
        for t in range(L):
            if W is None:
                Uv = S[:, 0]
            else:
                st = W > neg_p
                stay[:, t] = st
                Uv = S[:, t] + torch.where(st, W, neg_p)
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


def workload(T, D, K, a):
    import torch
    from abnet3_amd import _lib, kmeans
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    lab = torch.randint(0, K, (T // 8 + 1,), device='cuda', generator=g).repeat_interleave(8)[:T]      # 80 ms "phones"
    table = (centres[lab] + 1.5 * torch.randn(T, D, device='cuda', generator=g) + 5.0).contiguous()
    table, shift, good = kmeans.prepare(table, 'euclidean')
    mu = kmeans.initial_centroids(table, shift, good, K, 0)
    st = kmeans.LloydState(mu, T, table.device)
    for _ in range(3):
        kmeans.lloyd_iteration(table, shift, st)
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    n_utt, max_len = len(len_h), int(len_h.max())
    ws_bytes = int(lib.abn_kmeans_viterbi_ws_bytes(n_utt, max_len, K, D))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device='cuda')
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    obj = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    flop = 2.0 * T * K * (D + 1)
    res = {'T': T, 'D': D, 'K': K, 'utterances': n_utt, 'max_len': max_len, 'workspace_bytes': ws_bytes,
           'score_matrix_bytes_never_formed': 4 * T * K, 'flop_of_the_score_gemm': flop}
    pen = a.penalty

    def vit(penalty=pen):
        _lib.check(lib.abn_kmeans_viterbi(_lib.ptr(table), T, D, _lib.ptr(off), _lib.ptr(lens), n_utt, _lib.ptr(shift), _lib.ptr(st.m),
                                          _lib.ptr(st.b), K, float(np.float32(penalty / 2.0)), _lib.ptr(ids), _lib.ptr(obj), _lib.ptr(nsw),
                                          _lib.ptr(ws), ws.numel(), _lib.stream()), 'abn_kmeans_viterbi')

    plain = torch.empty(T, dtype=torch.int32, device='cuda')

    def floor():
        kmeans.assign(table, shift, st.m, st.b, ids=plain)

    xc = table - shift
    off64, len64 = off, lens.to(torch.int64)
    hold = {}

    def t_route():
        hold['ids'] = torch_viterbi(xc, st.m, st.b, off64, len64, float(np.float32(pen / 2.0)), a.utt_chunk)

    vit(), floor()
    res['abn_kmeans_viterbi'] = dict(median_ms(vit), penalty=pen)
    res['abn_kmeans_assign'] = median_ms(floor)
    res['torch_route'] = dict(median_ms(t_route, calls=a.torch_calls), calls=a.torch_calls, utterances_per_chunk=a.utt_chunk)
    res['abn_kmeans_viterbi_again'] = median_ms(vit)
    ms = res['abn_kmeans_viterbi']['median_ms']
    res['cells_per_s'] = round(T * K / (ms * 1e-3), 1)
    res['score_gemm_share_of_fp32_mfma_roof'] = round(flop / (ms * 1e-3) / FP32_MFMA_FLOPS, 4)
    res['time_over_assign_floor'] = round(ms / res['abn_kmeans_assign']['median_ms'], 3)
    res['speedup_over_torch_route'] = round(res['torch_route']['median_ms'] / ms, 3)
    vit()
    res['agreement'] = {'ids_that_differ_from_the_torch_route': int((ids.to(torch.int64) != hold['ids']).sum())}
    sweep = []
    for penalty in a.sweep:
        vit(penalty)
        host = ids.cpu().numpy()
        seqs = kmeans.unit_sequences({u: host[o:o + n] for u, (o, n) in enumerate(zip(off_h, len_h))})
        sweep.append({'penalty': penalty, 'switches': int(nsw.sum()), 'symbols': int(sum(len(v) for v in seqs.values())),
                      'bitrate_bits_per_s': round(kmeans.bitrate(seqs, T * FRAME_SECONDS), 2)})
    res['penalty_sweep'] = sweep
    del hold, xc
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--penalty', type=float, default=20.0, help='the penalty of the timed calls (units of the distortion)')
    ap.add_argument('--sweep', type=float, nargs='*', default=[0.0, 5.0, 20.0, 80.0])
    ap.add_argument('--utt-chunk', type=int, default=256, help='utterances per padded score tensor of the torch route')
    ap.add_argument('--torch-calls', type=int, default=15)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'units_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'fp32_mfma_roof_flops': FP32_MFMA_FLOPS,
           'workloads': [workload(a.frames, 40, 256, a), workload(a.frames, 40, 1024, a), workload(a.frames, 100, 1024, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
