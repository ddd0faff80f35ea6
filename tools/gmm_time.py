"""Times the Gaussian-mixture kernels (abnet3_amd/csrc/gmm.hip) and GmmPosteriorgram (abnet3_amd/gmm.py).

Workloads: the C5 frame count (1.14 M frames, tools/c5_corpus.py) as a synthetic mixture table, D = 39 with
K = 1024 and D = 40 with K = 256.  Timed, per workload:

  EM iteration     abn_gmm_posteriors (likelihoods only) + abn_gmm_accumulate + abn_gmm_mstep, and each of the three
                   on its own (device events)
  transform        abn_gmm_posteriors with the [T, K] output
  fit              GmmPosteriorgram.fit, --fit-iters iterations end to end (wall clock, read-backs included)
  torch route      the only way to do it before these kernels, same GPU, same process, alternating: the augmented
                   table [xc | xc^2 | 1] once, then per chunk of rows torch.mm + torch.logsumexp + exp + torch.mm for
                   the statistics (float64 accumulation over the chunks); its transform is mm + logsumexp + exp

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls; medians, minima and maxima are
reported.  The roofline is 2 T K (2D + 1) flop per GEMM -- one in the likelihood pass, two in the accumulate pass,
two in the transform (it sweeps twice) -- against the fp32 matrix-core rate (157.3 TFLOP/s).  HBM-side bytes per
launch need a counter run of rocprofv3 of their own and are not collected here.

python tools/gmm_time.py [--frames 1140000] [--fit-iters 5] [--out FILE]"""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

FP32_MFMA_FLOPS = 157.3e12
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
    return {'median_ms': round(float(np.median(ts)), 3), 'min_ms': round(float(min(ts)), 3), 'max_ms': round(float(max(ts)), 3)}


def torch_scores(aug, W, r0, r1):
    import torch
    S = torch.mm(aug[r0:r1], W.t())
    lse = torch.logsumexp(S, dim=1)
    return S, lse


def torch_iteration(aug, W, chunk):
    """E-step and statistics of the composition: (lse [T], sums [K, 2D + 1] float64)."""
    import torch
    T = aug.shape[0]
    sums = torch.zeros((W.shape[0], aug.shape[1]), dtype=torch.float64, device=aug.device)
    lses = []
    for r0 in range(0, T, chunk):
        r1 = min(T, r0 + chunk)
        S, lse = torch_scores(aug, W, r0, r1)
        g = torch.exp(S - lse[:, None])
        sums += torch.mm(g.t(), aug[r0:r1]).to(torch.float64)
        lses.append(lse)
    return torch.cat(lses), sums


def torch_transform(aug, W, out, chunk):
    import torch
    for r0 in range(0, aug.shape[0], chunk):
        r1 = min(aug.shape[0], r0 + chunk)
        S, lse = torch_scores(aug, W, r0, r1)
        torch.exp(S - lse[:, None], out=out[r0:r1])
    return out


def workload(T, D, K, a):
    import torch
    from abnet3_amd import _lib, gmm
    g = torch.Generator(device='cuda').manual_seed(D * 10000 + K)
    centres = 3.0 * torch.randn(K, D, device='cuda', generator=g)
    table = (centres[torch.randint(0, K, (T,), device='cuda', generator=g)] + torch.randn(T, D, device='cuda', generator=g)
             + 5.0).contiguous()
    shift, gv, good = gmm.training_moments(table)
    w, m, v = gmm.initial_parameters(table, shift, gv, good, K, 0)
    st = gmm.EMState(w, m, v, gv, table.device)
    lib = _lib.load()
    flop = 2.0 * T * K * (2 * D + 1)
    res = {'T': T, 'D': D, 'K': K, 'flop_per_gemm': flop, 'workspace_bytes': int(lib.abn_gmm_ws_bytes(T, K, D, 0))}
    A0, B0, c0 = st.A.clone(), st.B.clone(), st.c.clone()

    def reset():
        st.A.copy_(A0), st.B.copy_(B0), st.c.copy_(c0)

    def iteration():
        reset()
        gmm.em_iteration(table, shift, st)

    hold = {}

    def like():
        hold['lse'] = gmm.posteriors(table, shift, A0, B0, c0, want_post=False)[0]

    post = torch.empty((T, K), dtype=torch.float32, device='cuda')

    def transform():
        gmm.posteriors(table, shift, A0, B0, c0, want_post=True, out=post)

    iteration()
    ws = st.ws
    head = [_lib.ptr(table), T, D, _lib.ptr(shift), _lib.ptr(A0), _lib.ptr(B0), _lib.ptr(c0), K]
    like()

    def accumulate():
        _lib.check(lib.abn_gmm_accumulate(*(head + [_lib.ptr(hold['lse']), 0, _lib.ptr(ws), ws.numel(), _lib.stream()])), 'acc')

    A1, B1, c1 = torch.empty_like(A0), torch.empty_like(B0), torch.empty_like(c0)
    mu1, var1 = st.mu.clone(), st.var.clone()

    def mstep():
        _lib.check(lib.abn_gmm_mstep(_lib.ptr(ws), ws.numel(), _lib.ptr(hold['lse']), T, K, D, 0, _lib.ptr(st.gv), 0.01, 1.0,
                                     _lib.ptr(st.sums), _lib.ptr(st.w), _lib.ptr(mu1), _lib.ptr(var1), _lib.ptr(A1), _lib.ptr(B1),
                                     _lib.ptr(c1), _lib.ptr(st.stats), _lib.stream()), 'mstep')

    # the composition's inputs
    xc = table - shift
    aug = torch.cat([xc, xc * xc, torch.ones(T, 1, device='cuda')], dim=1).contiguous()
    W = torch.cat([A0, B0, c0[:, None]], dim=1).contiguous()

    def t_iteration():
        hold['t'] = torch_iteration(aug, W, a.chunk)

    def t_transform():
        torch_transform(aug, W, post, a.chunk)

    # alternating: fused, torch, fused, torch
    res['em_iteration'] = median_ms(iteration)
    res['torch_em_iteration'] = dict(median_ms(t_iteration), row_chunk=a.chunk)
    res['transform'] = median_ms(transform)
    res['torch_transform'] = dict(median_ms(t_transform), row_chunk=a.chunk)
    for name, fn, gemms in (('abn_gmm_posteriors_lse_only', like, 1), ('abn_gmm_accumulate', accumulate, 2), ('abn_gmm_mstep', mstep, 0)):
        r = median_ms(fn)
        if gemms:
            r['fraction_of_fp32_mfma_roof'] = round(gemms * flop / (r['median_ms'] * 1e-3) / FP32_MFMA_FLOPS, 4)
        res[name] = r
    res['transform']['fraction_of_fp32_mfma_roof'] = round(2 * flop / (res['transform']['median_ms'] * 1e-3) / FP32_MFMA_FLOPS, 4)
    res['transform']['bytes_written'] = 4 * T * K
    res['em_iteration_speedup_over_torch'] = round(res['torch_em_iteration']['median_ms'] / res['em_iteration']['median_ms'], 3)
    res['transform_speedup_over_torch'] = round(res['torch_transform']['median_ms'] / res['transform']['median_ms'], 3)
    # agreement of the two routes on the same tables
    iteration()
    lse_t, sums_t = hold['t']
    res['agreement'] = {'max_abs_lse_difference': float((hold['lse'] - lse_t).abs().max()),
                        'max_rel_statistics_difference': float(((st.sums - sums_t).abs() / sums_t.abs().clamp_min(1.0)).max())}
    del aug, post, hold
    torch.cuda.empty_cache()

    # fit end to end (wall clock): the model object's route, and the composition with the same M-step on the host
    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t0
    fit = lambda: gmm.GmmPosteriorgram(K, n_iter=a.fit_iters, tol=-np.inf).fit(table)
    fit()
    ts = [wall(fit) for _ in range(3)]
    res['fit_end_to_end'] = {'iterations': a.fit_iters, 'median_s': round(float(np.median(ts)), 4), 'min_s': round(min(ts), 4),
                             'max_s': round(max(ts), 4)}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--chunk', type=int, default=65536, help='rows per torch.mm of the composition')
    ap.add_argument('--fit-iters', type=int, default=5)
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'gmm_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'fp32_mfma_roof_flops': FP32_MFMA_FLOPS,
           'workloads': [workload(a.frames, 39, 1024, a), workload(a.frames, 40, 256, a)]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')


if __name__ == '__main__':
    main()
