"""Times the semi-Markov decoder with explicit unit durations (abnu_hmm_hsmm_viterbi, abnet3_amd/csrc/hmm_hsmm.hip) against
the full-transition decoders without them, and abnu_hmm_run_stats.

Workloads and protocol are tools/hmm_dense_decode_time.py's: its corpus (1.14 M frames as a synthetic clustered table, cut into
seeded utterances of 200 .. 1000 frames; the mixture is three EM iterations from the documented initialisation) at D = 40,
K = 64 and K = 128, the sticky matrix of the mixture's weights at stay 0.9 as the transition matrix and its geometric durations
(hmm.geometric_durations) at L = 8 and L = 32 as the duration law, device events around one launch for the corpus, every
route settling the clock (untimed calls for 0.3 s) before its 15 timed calls; medians, minima and maxima.  Timed per shape, in
one process and alternating:

  plain             abnz_hmm_dense_viterbi
  min_duration 8    abnw_hmm_dense_viterbi_dur(S = 8)
  durations L       abnu_hmm_hsmm_viterbi, and its ratios over the two medians taken just before it
  run statistics    abnu_hmm_run_stats on the ids it decoded
  torch             the same recurrence's FORWARD pass (scores, exit maxima, K x K max-plus, chain shift, normalisation; no
                    backpointers, no traceback) as a loop of batched torch ops over utterances padded to the longest of their
                    chunk, in the manner of tools/hmm_decode_time.py's torch_viterbi: 5 timed calls (each is seconds long)

Before anything is timed the new entry runs on exact inputs (integer frames, tables in eighths: every fp32 operation exact)
laid out as the timed corpus' first utterances, and every id, log_prob, n_switch and n_good must equal
tests/hmm_hsmm_np.py's, the run statistics of those ids its run_stats; and the torch loop's summed log_prob on the timed corpus
must agree with the kernel's to 1e-4 relative.  Otherwise the run reports failure and exits 1.

python tools/hmm_hsmm_time.py [--frames 1140000] [--stay 0.9] [--check-utterances 6] [--no-torch] [--out FILE]"""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))
SHAPES = ((64, 8), (64, 32), (128, 8), (128, 32))
MIN_DURATION = 8


def exact_check(off_h, len_h, n_check, D, K, L):
    """The new entries against the restatement on exact inputs laid out as the corpus' first n_check utterances."""
    import torch
    import hmm_hsmm_np as hs
    from abnet3_amd import hmm
    off, lens = off_h[:n_check], len_h[:n_check]
    T = int((off + lens).max())
    rng = np.random.default_rng(K + L)
    x = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    A = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = (rng.integers(-16, 17, size=K) / 8.0).astype(np.float32)
    li = (-rng.integers(0, 41, size=K) / 8.0).astype(np.float32)
    lx = (-rng.integers(0, 25, size=(K, K)) / 8.0).astype(np.float32)
    ld = (-rng.integers(0, 25, size=(K, L)) / 8.0).astype(np.float32)
    ls = (-rng.integers(0, 9, size=K) / 8.0).astype(np.float32)
    x64 = x.astype(np.float64)
    s64 = x64 @ A.astype(np.float64).T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)
    s = s64.astype(np.float32)
    if not np.array_equal(s.astype(np.float64), s64):
        return {'ok': False, 'why': 'the float32 scores of the exact inputs are not exact'}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = hmm.hsmm_viterbi(dev(x), off, lens, dev(np.zeros(D, dtype=np.float32)), dev(A), dev(B), dev(c0), dev(li), dev(lx), dev(ld),
                           dev(ls), ids=torch.full((T,), -7, dtype=torch.int32, device='cuda'))
    stats = hmm.run_stats(got[0], off, lens, K, L)
    torch.cuda.synchronize()
    ref = hs.viterbi(s, np.ones(T, dtype=bool), off, lens, li, lx, ld, ls)
    same = [bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(got, ref)]
    same_stats = [bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(stats, hs.run_stats(ref[0], off, lens, K, L))]
    return {'ok': all(same) and all(same_stats), 'max_duration': L, 'utterances': int(n_check), 'frames': int(lens.sum()),
            'ids_log_prob_n_switch_n_good_equal': same, 'dur_tail_equal': same_stats}


def torch_forward(xc, A, B, c0, li, lx, ld, ls, off, lens, utt_chunk):
    """The recurrence's forward pass in batched torch ops over padded utterances (no BAD frames here): the summed log_prob."""
    import torch
    T, K = xc.shape[0], A.shape[0]
    L = ld.shape[1]
    lxo = lx.masked_fill(torch.eye(K, dtype=torch.bool, device=xc.device), float('-inf'))
    total = torch.zeros((), dtype=torch.float64, device=xc.device)
    for u0 in range(0, len(lens), utt_chunk):
        o, n = off[u0:u0 + utt_chunk], lens[u0:u0 + utt_chunk]
        U, Lmax = len(n), int(n.max())
        rows = (o[:, None] + torch.arange(Lmax, device=xc.device)[None, :]).clamp_(max=T - 1)
        x = xc[rows.reshape(-1)]
        S = (torch.addmm(c0[None, :], x, A.t()) + torch.mm(x * x, B.t())).view(U, Lmax, K)
        del x
        lp = torch.zeros(U, dtype=torch.float64, device=xc.device)
        V = None
        for t in range(Lmax):
            s = S[:, t]
            if V is None:
                Un = torch.full((U, K, L), float('-inf'), device=xc.device)
                Un[:, :, 0] = s + li[None, :]
            else:
                xexit = (V + ld[None]).max(dim=2).values                              # [U, K]
                ent = (xexit[:, :, None] + lxo[None]).max(dim=1).values             # [U, K]
                tail = torch.maximum(V[:, :, L - 1] + ls[None, :], V[:, :, L - 2])
                Un = torch.cat([ent[:, :, None], V[:, :, :L - 2], tail[:, :, None]], dim=2) + s[:, :, None]
            N = Un.amax(dim=(1, 2))
            live = n > t
            Vn = Un - N[:, None, None]
            V = Vn if V is None else torch.where(live[:, None, None], Vn, V)
            lp += torch.where(live, N.to(torch.float64), torch.zeros_like(lp))
        lp += (V + ld[None]).amax(dim=(1, 2)).to(torch.float64)
        total += lp.sum()
    return total


def workload(T, D, K, L, a):
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
    shift, A, B, c0, _ = sticky.device_tables(table.device)
    init_h, trans_h = hmm.sticky_transitions(model.weights_, a.stay)
    up = lambda t: torch.from_numpy(np.ascontiguousarray(t)).cuda()
    li, lt = (up(t) for t in hmm.log_transitions(init_h, trans_h))
    lx = up(hmm.switch_log_transitions(init_h, trans_h)[1])
    ld, ls = (up(t) for t in hmm.duration_tables(*hmm.geometric_durations(trans_h, L)))
    off_h, len_h = cut(T, D + K)
    res = {'T': T, 'D': D, 'K': K, 'max_duration': L, 'stay': float(np.float32(a.stay)), 'utterances': len(len_h),
           'max_len': int(len_h.max())}
    res['exact_check'] = exact_check(off_h, len_h, a.check_utterances, D, K, L)
    if not res['exact_check']['ok']:
        return res
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib, p = _lib.load(), _lib.ptr
    n_utt, max_len = len(len_h), int(len_h.max())
    sizes = {'plain': int(lib.abnz_hmm_dense_viterbi_ws_bytes(n_utt, max_len, K, D)),
             'min_duration': int(lib.abnw_hmm_dense_viterbi_dur_ws_bytes(n_utt, max_len, K, D)),
             'durations': int(lib.abnu_hmm_hsmm_viterbi_ws_bytes(n_utt, max_len, K, D, L))}
    res['workspace_bytes'] = sizes
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device='cuda')
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    lp = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    dur = torch.empty((K, L), dtype=torch.int64, device='cuda')
    tail = torch.empty(K, dtype=torch.int64, device='cuda')
    head = (p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(li))
    outs = (K, p(ids), p(lp), p(nsw), p(ng), p(ws))

    def plain():
        _lib.check(lib.abnz_hmm_dense_viterbi(*(head + (p(lt),) + outs + (sizes['plain'], _lib.stream()))), 'abnz_hmm_dense_viterbi')

    def min_duration():
        _lib.check(lib.abnw_hmm_dense_viterbi_dur(*(head + (p(lt),) + outs + (sizes['min_duration'], _lib.stream(), MIN_DURATION))),
                   'abnw_hmm_dense_viterbi_dur')

    def durations():
        _lib.check(lib.abnu_hmm_hsmm_viterbi(*(head + (p(lx),) + outs + (sizes['durations'], _lib.stream(), p(ld), p(ls), L))),
                   'abnu_hmm_hsmm_viterbi')

    def run_statistics():
        _lib.check(lib.abnu_hmm_run_stats(p(ids), T, p(off), p(lens), n_utt, K, L, p(dur), p(tail), _lib.stream()), 'abnu_hmm_run_stats')

    plain(), min_duration(), durations()
    t0 = median_ms(plain)
    t1 = median_ms(min_duration)
    t2 = median_ms(durations)
    torch.cuda.synchronize()
    kernel_lp = float(lp.sum())
    res.update({'plain': t0, 'min_duration_%d' % MIN_DURATION: t1, 'durations': t2,
                'over_plain': round(t2['median_ms'] / t0['median_ms'], 3), 'over_min_duration': round(t2['median_ms'] / t1['median_ms'], 3),
                'us_per_frame_of_a_workgroup': round(t2['median_ms'] * 1e3 / T * min(n_utt, 256), 4),
                'switches': int(nsw.sum()), 'mean_score_per_frame': kernel_lp / float(ng.sum())})
    res['run_stats'] = median_ms(run_statistics)
    torch.cuda.synchronize()
    res['runs'] = int(dur.sum())
    res['runs_are_the_segments'] = bool(int(dur.sum()) == int(nsw.sum()) + n_utt)
    if not a.no_torch:
        xc = table - shift[None, :]
        off64, lens64 = off, lens.to(torch.int64)
        route = lambda: torch_forward(xc, A, B, c0, li, lx, ld, ls, off64, lens64, a.utt_chunk)
        torch_lp = float(route())
        res['torch_forward'] = median_ms(route, calls=5)
        res['torch_forward_over_durations'] = round(res['torch_forward']['median_ms'] / t2['median_ms'], 2)
        res['torch_log_prob_relative_difference'] = abs(torch_lp - kernel_lp) / abs(kernel_lp)
    print('D = %d, K = %d, L = %d: plain %.3f ms, min_duration %d %.3f ms, durations %.3f ms (%.3f x, %.3f x), run_stats %.3f ms%s'
          % (D, K, L, t0['median_ms'], MIN_DURATION, t1['median_ms'], t2['median_ms'], res['over_plain'], res['over_min_duration'],
             res['run_stats']['median_ms'], '' if a.no_torch else ', torch forward %.1f ms' % res['torch_forward']['median_ms']),
          file=sys.stderr, flush=True)
    del ws
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--check-utterances', type=int, default=6)
    ap.add_argument('--utt-chunk', type=int, default=512, help='utterances of one padded batch of the torch loop')
    ap.add_argument('--no-torch', action='store_true', help='leave the torch loop out')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_hsmm_time.json'))
    a = ap.parse_args()
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'torch_calls_per_median': 5, 'workloads': []}
    for K, L in SHAPES:
        res['workloads'].append(workload(a.frames, 40, K, L, a))
        w = res['workloads'][-1]
        if not w['exact_check']['ok']:
            res['failed'] = 'the new entries differ from tests/hmm_hsmm_np.py on exact inputs (K = %d, L = %d)' % (K, L)
            break
        if not w['runs_are_the_segments']:
            res['failed'] = 'the runs abnu_hmm_run_stats counts are not the decoder\'s segments (K = %d, L = %d)' % (K, L)
            break
        if not a.no_torch and not w['torch_log_prob_relative_difference'] <= 1e-4:
            res['failed'] = 'the torch loop and the kernel disagree on the summed log_prob (K = %d, L = %d)' % (K, L)
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
