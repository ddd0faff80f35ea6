"""Times the minimum unit duration of the full-transition HMM's max-product path (abnw_hmm_dense_viterbi_dur,
abnet3_amd/csrc/hmm_dense_vit.hip) against the path without it (abnz_hmm_dense_viterbi).

Workloads and protocol are tools/hmm_dense_decode_time.py's: its corpus (1.14 M frames as a synthetic clustered table, cut
into seeded utterances of 200 .. 1000 frames; the mixture is three EM iterations from the documented initialisation) at
(D, K) = (40, 64), (40, 128), the sticky matrix of the mixture's weights at stay 0.9 as the transition matrix, device events
around one launch for the corpus, every route settling the clock (untimed calls for 0.3 s) before its 15 timed calls; medians,
minima and maxima.  Timed per workload, in one process and alternating, for S = 1, 2, 3, 5, 8:

  twin              abnz_hmm_dense_viterbi
  min_duration S    abnw_hmm_dense_viterbi_dur(S), and its ratio over the twin's median taken just before it

S = 1 launches the twin's kernel in the new entry's regions, so its ratio is the noise of the comparison.

abnz_hmm_dense_viterbi against another build of the library -- the commit before this entry existed (--parent-lib, a
libabnet3_hip.so built from it; ABNET3_HIP_LIB) --: a library is bound once per process, so fresh child processes alternate
(that build, this build, that build, this build), each timing the twin alone on the same workloads three times; the medians of
each build, their spread, and the ratio of the builds' middle medians are reported.  Without such a library: null.

Before anything is timed the new entry runs on exact inputs (integer frames, tables in eighths: every fp32 operation exact)
laid out as the timed corpus' first utterances at S = 3, and every id, log_prob, n_switch and n_good must equal
tests/hmm_dense_dur_np.py's; at S = 1 its outputs must be the twin's bit for bit on the timed corpus.  Otherwise the run
reports failure and exits 1.

python tools/hmm_dense_dur_time.py [--frames 1140000] [--stay 0.9] [--check-utterances 6] [--parent-lib LIB] [--out FILE]"""
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
DURATIONS = (1, 2, 3, 5, 8)


def exact_check(off_h, len_h, n_check, D, K, S):
    """The new entry against the restatement on exact inputs laid out as the corpus' first n_check utterances."""
    import torch
    import hmm_dense_dur_np as dd
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
                            ids=torch.full((T,), -7, dtype=torch.int32, device='cuda'), min_duration=S)
    torch.cuda.synchronize()
    ref = dd.viterbi(s, np.ones(T, dtype=bool), off, lens, li, lt, S)
    same = [bool(np.array_equal(g.cpu().numpy(), r)) for g, r in zip(got, ref)]
    return {'ok': all(same), 'min_duration': S, 'utterances': int(n_check), 'frames': int(lens.sum()),
            'ids_log_prob_n_switch_n_good_equal': same}


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
    lw_h, ls_h, lr_h = hmm.viterbi_tables(model.weights_, a.stay)
    lt_h = np.repeat(lr_h[None, :], K, axis=0)
    lt_h[np.arange(K), np.arange(K)] = ls_h
    li, lt = (torch.from_numpy(np.ascontiguousarray(t)).cuda() for t in (lw_h, lt_h))
    off_h, len_h = cut(T, D + K)
    res = {'T': T, 'D': D, 'K': K, 'stay': float(np.float32(a.stay)), 'utterances': len(len_h), 'max_len': int(len_h.max())}
    if not a.twin_only:
        res['exact_check'] = exact_check(off_h, len_h, a.check_utterances, D, K, 3)
        if not res['exact_check']['ok']:
            return res
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib, p = _lib.load(), _lib.ptr
    n_utt, max_len = len(len_h), int(len_h.max())
    size_twin = int(lib.abnz_hmm_dense_viterbi_ws_bytes(n_utt, max_len, K, D))
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    lp = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ws = torch.empty(size_twin, dtype=torch.uint8, device='cuda')

    def twin():
        _lib.check(lib.abnz_hmm_dense_viterbi(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(li), p(lt), K,
                                              p(ids), p(lp), p(nsw), p(ng), p(ws), size_twin, _lib.stream()), 'abnz_hmm_dense_viterbi')

    if a.twin_only:                                      # (a child of --parent-lib: the twin alone, three times)
        twin()
        res['twin'] = [median_ms(twin) for _ in range(3)]
        return res
    size_dur = int(lib.abnw_hmm_dense_viterbi_dur_ws_bytes(n_utt, max_len, K, D))
    res['workspace_bytes'] = {'twin': size_twin, 'min_duration': size_dur}
    ws2 = torch.empty(size_dur, dtype=torch.uint8, device='cuda')
    ids2 = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    lp2 = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw2 = torch.zeros(n_utt, dtype=torch.int32, device='cuda')

    def dur(S):
        def call():
            _lib.check(lib.abnw_hmm_dense_viterbi_dur(p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(li), p(lt),
                                                      K, p(ids2), p(lp2), p(nsw2), p(ng), p(ws2), size_dur, _lib.stream(), S),
                       'abnw_hmm_dense_viterbi_dur')
        return call

    twin(), dur(1)()
    torch.cuda.synchronize()
    res['min_duration_1_is_the_twin_bit_for_bit'] = bool(torch.equal(ids, ids2) and torch.equal(lp.view(torch.int64), lp2.view(torch.int64))
                                                         and torch.equal(nsw, nsw2))
    if not res['min_duration_1_is_the_twin_bit_for_bit']:
        return res
    res['by_min_duration'] = []
    for S in DURATIONS:
        dur(S)()
        t0 = median_ms(twin)
        t1 = median_ms(dur(S))
        torch.cuda.synchronize()
        res['by_min_duration'].append({'min_duration': S, 'twin': t0, 'min_duration_entry': t1,
                                       'over_twin': round(t1['median_ms'] / t0['median_ms'], 3),
                                       'us_per_frame_of_a_workgroup': round(t1['median_ms'] * 1e3 / T * min(n_utt, 256), 4),
                                       'switches': int(nsw2.sum()), 'mean_score_per_frame': float(lp2.sum() / ng.sum())})
        print('D = %d, K = %d, S = %d: twin %.3f ms, min_duration %.3f ms (%.3f x)'
              % (D, K, S, t0['median_ms'], t1['median_ms'], t1['median_ms'] / t0['median_ms']), file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    return res


def twin_in_a_child(a, lib_path):
    """The twin's medians on both workloads in a fresh process bound to lib_path (None: this build)."""
    env = dict(os.environ)
    if lib_path is not None:
        env['ABNET3_HIP_LIB'] = os.path.abspath(lib_path)
    child = subprocess.run([sys.executable, os.path.abspath(__file__), '--twin-only', '--frames', str(a.frames), '--stay', str(a.stay)],
                           env=env, stdout=subprocess.PIPE, text=True, timeout=600)
    if child.returncode != 0:
        return None
    return [[m['median_ms'] for m in w['twin']] for w in json.loads(child.stdout.strip().splitlines()[-1])['workloads']]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--check-utterances', type=int, default=6)
    ap.add_argument('--parent-lib', default=os.path.join(ROOT, 'tools', 'variants', 'lib_parent.so'),
                    help='libabnet3_hip.so built from the commit before abnw_hmm_dense_viterbi_dur; missing: that comparison is null')
    ap.add_argument('--twin-only', action='store_true', help='(a child) time abnz_hmm_dense_viterbi alone, no checks, no file')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'hmm_dense_dur_time.json'))
    a = ap.parse_args()
    if a.twin_only:
        from abnet3_amd import _lib
        _lib.NEXT4_SYMBOLS.clear()                       # the other build does not export them, and this route calls none
        import torch
        res = {'device': torch.cuda.get_device_name(0), 'workloads': [workload(a.frames, D, K, a) for D, K in ((40, 64), (40, 128))]}
        print(json.dumps(res))
        return 0
    against_parent = None
    if os.path.exists(a.parent_lib):
        # first, in processes of their own that end before this one touches the device
        runs = {'parent': [], 'this': []}
        for which in ('parent', 'this', 'parent', 'this'):
            got = twin_in_a_child(a, a.parent_lib if which == 'parent' else None)
            if got is None:
                print('FAILED: a child process timing the twin (%s build) failed' % which, file=sys.stderr)
                return 1
            runs[which].append(got)
        against_parent = []
        for i in range(2):
            par = sorted(m for r in runs['parent'] for m in r[i])
            new = sorted(m for r in runs['this'] for m in r[i])
            against_parent.append({'parent_medians_ms': par, 'this_medians_ms': new,
                                   'this_over_parent': round(float(np.median(new) / np.median(par)), 4),
                                   'spread_of_a_build': round(max(par[-1] / par[0], new[-1] / new[0]) - 1.0, 4)})
    import torch
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'workloads': []}
    for i, (D, K) in enumerate(((40, 64), (40, 128))):
        res['workloads'].append(workload(a.frames, D, K, a))
        w = res['workloads'][-1]
        if not w['exact_check']['ok']:
            res['failed'] = 'the new entry differs from tests/hmm_dense_dur_np.py on exact inputs (D = %d, K = %d)' % (D, K)
            break
        if not w['min_duration_1_is_the_twin_bit_for_bit']:
            res['failed'] = 'min_duration = 1 differs from abnz_hmm_dense_viterbi (D = %d, K = %d)' % (D, K)
            break
        w['twin_against_the_parent_build'] = None if against_parent is None else against_parent[i]
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
