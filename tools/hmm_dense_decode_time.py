"""Times the max-product path of the full-transition HMM (abnz_hmm_dense_viterbi, abnet3_amd/csrc/hmm_dense_vit.hip).

Workloads: tools/hmm_time.py's corpus (1.14 M frames as a synthetic clustered table, cut into the same kind of seeded
utterances of 200 .. 1000 frames; the mixture is three EM iterations from the documented initialisation) at
(D, K) = (40, 64), (40, 128).  The transition matrix is the sticky matrix of the mixture's weights at stay 0.9, so the two
yardsticks compute the same model (the decoder reads the sticky decoder's own log tables laid out as a matrix, and its
log_prob must equal abn_hmm_viterbi's bit for bit, or the run reports failure).  Timed, per workload, in the same process
and alternating:

  dense decode      abnz_hmm_dense_viterbi, one launch for the corpus (device events)
  filter sweep      abny_hmm_dense_forward_backward(mode = 1): the same score phase and one K' x K' product per frame
  sticky decode     abn_hmm_viterbi on the sticky log tables of the same model

Every route settles the clock (untimed calls for 0.3 s) before its 15 timed calls; medians, minima and maxima are
reported, with the two ratios, microseconds per frame of a workgroup's utterances and the workspace bytes.

The traceback runs inside the one launch, so its share is taken from a variant of the library built without it
(`tools/variants.sh hmm_dense_vit "-DHDV_NO_TRACEBACK"` -> tools/variants/lib_HDV_NO_TRACEBACK.so, --without-traceback-lib):
a fresh child process loads that library (ABNET3_HIP_LIB), times the decoder alone on the same workloads with the same
protocol, and the share is 1 - without / with.  Without such a library the share is reported as null.

Before anything is timed the decoder runs on exact inputs (integer frames, tables in eighths: every fp32 operation exact)
laid out as the timed corpus' first utterances, and every id, log_prob, n_switch and n_good must equal
tests/hmm_dense_vit_np.py's; otherwise the run reports failure and exits 1.

python tools/hmm_dense_decode_time.py [--frames 1140000] [--stay 0.9] [--check-utterances 6] [--without-traceback-lib LIB] [--out FILE]"""
import argparse
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from gmm_time import median_ms
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, 'tests'))


def exact_check(off_h, len_h, n_check, D, K):
    """The decoder against the restatement on exact inputs laid out as the corpus' first n_check utterances."""
    import torch
    import hmm_dense_vit_np as dv
    from abnet3_amd import hmm
    off, lens = off_h[:n_check], len_h[:n_check]
    T = int((off + lens).max())
    rng = np.random.default_rng(K)
    x = rng.integers(-3, 4, size=(T, D)).astype(np.float32)
    A = rng.integers(-2, 3, size=(K, D)).astype(np.float32)
    B = np.full((K, D), -0.5, dtype=np.float32)
    c0 = (rng.integers(-16, 17, size=K) / 8.0).astype(np.float32)
    li = (-rng.integers(0, 41, size=K) / 8.0).astype(np.float32)
    lt = (-rng.integers(0, 25, size=(K, K)) / 8.0).astype(np.float32)
    x64 = x.astype(np.float64)
    s64 = x64 @ A.astype(np.float64).T + (x64 * x64) @ B.astype(np.float64).T + c0.astype(np.float64)
    s = s64.astype(np.float32)
    if not np.array_equal(s.astype(np.float64), s64):
        return {'ok': False, 'why': 'the float32 scores of the exact inputs are not exact'}
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    got = hmm.dense_viterbi(dev(x), off, lens, dev(np.zeros(D, dtype=np.float32)), dev(A), dev(B), dev(c0), dev(li), dev(lt),
                            ids=torch.full((T,), -7, dtype=torch.int32, device='cuda'))
    torch.cuda.synchronize()
    ref = dv.viterbi(s, np.ones(T, dtype=bool), off, lens, li, lt)
    same = [bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(got, ref)]
    return {'ok': all(same), 'utterances': int(n_check), 'frames': int(lens.sum()), 'ids_log_prob_n_switch_n_good_equal': same}


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
    shift, A, B, c0, _ = sticky.device_tables(table.device)
    init_h, trans_h = hmm.sticky_transitions(model.weights_, a.stay)
    init, trans = torch.from_numpy(init_h).cuda(), torch.from_numpy(trans_h).cuda()
    # the decoder's tables are the sticky decoder's own (lt[j][k] = lr[k] off the diagonal, ls[k] on it; li = lw): the same
    # float32 numbers, so the two decoders must give the same log_prob bit for bit (hmm.log_transitions(init, trans) would
    # take the logarithm of the rounded sum r + (1 - r) w instead: the same model up to one rounding)
    lw_h, ls_h, lr_h = hmm.viterbi_tables(model.weights_, a.stay)
    lt_h = np.repeat(lr_h[None, :], K, axis=0)
    lt_h[np.arange(K), np.arange(K)] = ls_h
    lw, ls, lr, lt = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (lw_h, ls_h, lr_h, lt_h))
    li = lw
    off_h, len_h = cut(T, D + K)
    res = {'T': T, 'D': D, 'K': K, 'stay': float(np.float32(a.stay)), 'utterances': len(len_h), 'max_len': int(len_h.max())}
    if not a.decode_only:
        res['exact_check'] = exact_check(off_h, len_h, a.check_utterances, D, K)
        if not res['exact_check']['ok']:
            return res
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib, p = _lib.load(), _lib.ptr
    n_utt, max_len = len(len_h), int(len_h.max())
    sizes = {'dense_decode': int(lib.abnz_hmm_dense_viterbi_ws_bytes(n_utt, max_len, K, D)),
             'filter_sweep': int(lib.abny_hmm_dense_ws_bytes(n_utt, max_len, K, D)),
             'sticky_decode': int(lib.abn_hmm_viterbi_ws_bytes(n_utt, max_len, K, D))}
    res['workspace_bytes'] = sizes
    ws = torch.empty(max(sizes.values()), dtype=torch.uint8, device='cuda')
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    ids2 = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    post = torch.zeros((T, K), dtype=torch.float32, device='cuda')
    lp = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    lp2 = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    ll = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    nsw2 = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')

    def decode():
        _lib.check(lib.abnz_hmm_dense_viterbi(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(li), p(lt), K,
                                              p(ids), p(lp), p(nsw), p(ng), p(ws), sizes['dense_decode'], _lib.stream()),
                   'abnz_hmm_dense_viterbi')

    def filt():
        _lib.check(lib.abny_hmm_dense_forward_backward(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(init),
                                                       p(trans), K, 1, p(post), p(ll), p(ng), p(None), p(ws), sizes['filter_sweep'],
                                                       _lib.stream()), 'abny_hmm_dense_forward_backward')

    def sticky_decode():
        _lib.check(lib.abn_hmm_viterbi(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(lw), p(ls), p(lr), K,
                                       p(ids2), p(lp2), p(nsw2), p(ng), p(ws), sizes['sticky_decode'], _lib.stream()), 'abn_hmm_viterbi')

    if a.decode_only:                                    # (the child of --without-traceback-lib: the decoder alone, twice)
        decode()
        res['dense_decode'] = median_ms(decode)
        res['dense_decode_again'] = median_ms(decode)
        return res
    decode(), filt(), sticky_decode()
    res['dense_decode'] = median_ms(decode)
    res['filter_sweep'] = median_ms(filt)
    res['sticky_decode'] = median_ms(sticky_decode)
    res['dense_decode_again'] = median_ms(decode)
    res['filter_sweep_again'] = median_ms(filt)
    dd, fs, sd = (res[k]['median_ms'] for k in ('dense_decode', 'filter_sweep', 'sticky_decode'))
    res['decode_over_filter_sweep'] = round(dd / fs, 3)
    res['decode_over_sticky_decode'] = round(dd / sd, 3)
    res['us_per_frame_of_a_workgroup'] = round(dd * 1e3 / T * min(n_utt, 256), 4)
    res['traceback_share'] = None
    decode(), sticky_decode()
    torch.cuda.synchronize()
    # the same tables through both decoders: log_prob bit for bit (tests/test_gpu_hmm_dense_vit.py), the ids up to ties
    res['agreement_with_the_sticky_decoder'] = {
        'log_prob_bit_equal': bool(torch.equal(lp.view(torch.int64), lp2.view(torch.int64))),
        'ids_that_differ': int((ids != ids2).sum()), 'switches': int(nsw.sum()), 'sticky_switches': int(nsw2.sum()),
        'mean_log_prob_per_frame': float(lp.sum() / ng.sum())}
    print('D = %d, K = %d: dense decode %.3f ms, filter sweep %.3f ms, sticky decode %.3f ms' % (D, K, dd, fs, sd), file=sys.stderr, flush=True)
    del post
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--check-utterances', type=int, default=6)
    ap.add_argument('--without-traceback-lib', default=os.path.join(ROOT, 'tools', 'variants', 'lib_HDV_NO_TRACEBACK.so'),
                    help='a build of the library with -DHDV_NO_TRACEBACK (tools/variants.sh); missing: the share is null')
    ap.add_argument('--decode-only', action='store_true', help='(the child) time the decoder alone, no checks, no file')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_dense_decode_time.json'))
    a = ap.parse_args()
    bare = None
    if not a.decode_only and os.path.exists(a.without_traceback_lib):
        # first, and in a process of its own that ends before this one touches the device: a library is bound once per process
        child = subprocess.run([sys.executable, os.path.abspath(__file__), '--decode-only', '--frames', str(a.frames), '--stay', str(a.stay)],
                               env=dict(os.environ, ABNET3_HIP_LIB=os.path.abspath(a.without_traceback_lib)), stdout=subprocess.PIPE,
                               text=True, timeout=600)
        if child.returncode != 0:
            print('FAILED: the run without the traceback ended with %d' % child.returncode, file=sys.stderr)
            return 1
        bare = json.loads(child.stdout.strip().splitlines()[-1])['workloads']
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'workloads': []}
    if a.decode_only:
        res['workloads'] = [workload(a.frames, D, K, a) for D, K in ((40, 64), (40, 128))]
        print(json.dumps(res))
        return 0
    for D, K in ((40, 64), (40, 128)):
        res['workloads'].append(workload(a.frames, D, K, a))
        if not res['workloads'][-1]['exact_check']['ok']:
            res['failed'] = 'the decoder differs from tests/hmm_dense_vit_np.py on exact inputs (D = %d, K = %d)' % (D, K)
            break
        if not res['workloads'][-1]['agreement_with_the_sticky_decoder']['log_prob_bit_equal']:
            res['failed'] = 'log_prob differs from abn_hmm_viterbi on the same tables (D = %d, K = %d)' % (D, K)
            break
    if 'failed' not in res and bare is not None:
        for w, b in zip(res['workloads'], bare):
            w['dense_decode_without_traceback'] = b['dense_decode']
            w['traceback_share'] = round(1.0 - b['dense_decode']['median_ms'] / w['dense_decode']['median_ms'], 4)
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
