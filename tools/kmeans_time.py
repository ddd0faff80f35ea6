"""Times the k-means kernels (abnet3_amd/csrc/kmeans.hip) and KMeansQuantizer (abnet3_amd/kmeans.py).

Workloads: the C5 frame count (1.14 M frames, tools/c5_corpus.py) as a synthetic clustered table, D = 40 with
K = 256 and K = 1024, and D = 100 with K = 1024.  Timed, per workload:

  Lloyd iteration  abn_kmeans_assign + abn_kmeans_accumulate + abn_kmeans_update, and each of the three on its own
                   (device events)
  predict          abn_kmeans_assign alone, as KMeansQuantizer.predict calls it
  torch route (a)  the only way to do it before these kernels, same GPU, same process, alternating: per chunk of rows
                   torch.mm + argmax, then index_add_ of the rows and the counts (floating-point atomics: not
                   reproducible); its predict is mm + argmax
  mixture (b)      gmm.em_iteration of the existing mixture at the same T, K, D (D <= 127 only): one iteration of the
                   soft model, which does strictly more matrix work

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls; medians, minima and maxima are
reported.  The roofline of the assign pass is 2 T K (D + 1) flop against the fp32 matrix-core rate (157.3 TFLOP/s); the
accumulate pass is reported against the bytes it must move (the rows once, the ids once per centroid tile, the
partials once) at 6.3 TB/s.

python tools/kmeans_time.py [--frames 1140000] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import FP32_MFMA_FLOPS, median_ms

HBM_BYTES_PER_S = 6.3e12
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def torch_assign(xc, m, b, chunk):
    import torch
    ids = []
    for r0 in range(0, xc.shape[0], chunk):
        ids.append(torch.argmax(torch.addmm(b[None, :], xc[r0:r0 + chunk], m.t()), dim=1))
    return torch.cat(ids)


def torch_iteration(xc, m, b, chunk):
    """Assignment and statistics of the composition: (ids [T], S [K, D], N [K])."""
    import torch
    ids = torch_assign(xc, m, b, chunk)
    S = torch.zeros_like(m).index_add_(0, ids, xc)
    N = torch.zeros(m.shape[0], device=m.device).index_add_(0, ids, torch.ones(xc.shape[0], device=m.device))
    return ids, S, N, S / N.clamp_min(1.0)[:, None]


def workload(T, D, K, a):
    import torch
    from abnet3_amd import _lib, gmm, kmeans
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    table = (centres[torch.randint(0, K, (T,), device='cuda', generator=g)] + torch.randn(T, D, device='cuda', generator=g)
             + 5.0).contiguous()
    table, shift, good = kmeans.prepare(table, 'euclidean')
    mu = kmeans.initial_centroids(table, shift, good, K, 0)
    st = kmeans.LloydState(mu, T, table.device)
    lib = _lib.load()
    flop = 2.0 * T * K * (D + 1)
    ws_bytes = int(lib.abn_kmeans_ws_bytes(T, K, D, 0))
    res = {'T': T, 'D': D, 'K': K, 'flop_of_the_assign_gemm': flop, 'workspace_bytes': ws_bytes}
    mu0, m0, b0 = st.mu.clone(), st.m.clone(), st.b.clone()

    def iteration():
        st.mu.copy_(mu0), st.m.copy_(m0), st.b.copy_(b0)
        kmeans.lloyd_iteration(table, shift, st)

    def predict():
        kmeans.assign(table, shift, m0, b0, ids=st.ids)

    iteration()
    predict()
    mu1, m1, b1 = mu0.clone(), m0.clone(), b0.clone()

    def accumulate():
        _lib.check(lib.abn_kmeans_accumulate(_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(m0), K, _lib.ptr(st.ids), 0,
                                             _lib.ptr(st.ws), st.ws.numel(), _lib.stream()), 'accumulate')

    def update():
        _lib.check(lib.abn_kmeans_update(_lib.ptr(st.ws), st.ws.numel(), _lib.ptr(st.ids), T, K, D, 0, 0, _lib.ptr(st.sums),
                                         _lib.ptr(mu1), _lib.ptr(m1), _lib.ptr(b1), _lib.ptr(st.stats), _lib.stream()), 'update')

    xc = table - shift
    hold = {}

    def t_iteration():
        hold['t'] = torch_iteration(xc, m0, b0, a.chunk)

    def t_predict():
        hold['p'] = torch_assign(xc, m0, b0, a.chunk)

    # alternating: fused, torch, fused, torch
    res['lloyd_iteration'] = median_ms(iteration)
    res['torch_iteration'] = dict(median_ms(t_iteration), row_chunk=a.chunk)
    res['predict'] = median_ms(predict)
    res['torch_predict'] = dict(median_ms(t_predict), row_chunk=a.chunk)
    res['abn_kmeans_assign'] = dict(res['predict'])
    res['abn_kmeans_assign']['fraction_of_fp32_mfma_roof'] = round(flop / (res['predict']['median_ms'] * 1e-3) / FP32_MFMA_FLOPS, 4)
    accumulate()
    res['abn_kmeans_accumulate'] = median_ms(accumulate)
    tiles = -(-K // max(16, min(128, 1 << int(np.floor(np.log2(8192 / D))))))
    moved = 4.0 * T * D + 4.0 * T * tiles + ws_bytes
    res['abn_kmeans_accumulate'].update(bytes_moved=moved, centroid_tiles=int(tiles), fraction_of_hbm_rate=round(
        moved / (res['abn_kmeans_accumulate']['median_ms'] * 1e-3) / HBM_BYTES_PER_S, 4))
    res['abn_kmeans_update'] = median_ms(update)
    res['iteration_speedup_over_torch'] = round(res['torch_iteration']['median_ms'] / res['lloyd_iteration']['median_ms'], 3)
    res['predict_speedup_over_torch'] = round(res['torch_predict']['median_ms'] / res['predict']['median_ms'], 3)
    # agreement of the two routes on the same tables
    iteration()
    ids_t, _, N_t, mean_t = hold['t']
    live = N_t > 0
    res['agreement'] = {'ids_that_differ': int((st.ids.to(torch.int64) != ids_t).sum()),
                        'max_abs_centroid_difference': float((st.mu.to(torch.float32)[live] - mean_t[live]).abs().max())}
    del hold, xc
    torch.cuda.empty_cache()

    if D <= gmm.max_d():
        sh, gv, gd = gmm.training_moments(table)
        est = gmm.EMState(*gmm.initial_parameters(table, sh, gv, gd, K, 0), gv, table.device)
        A0, B0, c0 = est.A.clone(), est.B.clone(), est.c.clone()

        def em():
            est.A.copy_(A0), est.B.copy_(B0), est.c.copy_(c0)
            gmm.em_iteration(table, sh, est)

        em()
        res['gmm_em_iteration'] = median_ms(em)
        res['lloyd_iteration_again'] = median_ms(iteration)                  # (alternating: the quantiser once more)
        res['iteration_speedup_over_gmm_em'] = round(res['gmm_em_iteration']['median_ms'] / res['lloyd_iteration_again']['median_ms'], 3)
    else:
        res['gmm_em_iteration'] = 'not applicable: D > %d' % gmm.max_d()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--chunk', type=int, default=65536, help='rows per torch.mm of the composition')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'kmeans_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'fp32_mfma_roof_flops': FP32_MFMA_FLOPS,
           'hbm_bytes_per_s': HBM_BYTES_PER_S,
           'workloads': [workload(a.frames, 40, 256, a), workload(a.frames, 40, 1024, a), workload(a.frames, 100, 1024, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
