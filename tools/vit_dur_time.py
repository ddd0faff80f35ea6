"""Times the two max-product decoders with a minimum unit duration (abnx_kmeans_viterbi_dur, abnx_hmm_viterbi_dur:
abnet3_amd/csrc/kmeans.hip, hmm.hip, vit_wave.h) against the entries without one.

Workloads and protocol: tools/hmm_decode_time.py's and tools/units_time.py's (1.14 M frames as a synthetic clustered
table, D = 40 with K = 256 and K = 1024, D = 100 with K = 1024, the same seeded utterances of 200 .. 1000 frames, the
mixture of three EM iterations at stay 0.9 and the centroids of three Lloyd iterations at penalty 6); every route settles
the clock (untimed calls for 0.3 s) before its 15 timed calls (device events); medians.  Per workload and decoder, in one
process:

  new entry at S = 1, 2, 3, 5, 8   each alternating with the old entry at the same shape (`--repeats` medians each): the
                                   ratio new / old per S -- at S = 1 the price of the new kernel for the old result, whose
                                   outputs are compared bit for bit -- and the new entry's time against S
  --parent-lib FILE                the OLD entries of another build of the library (the parent commit's) alternating with
                                   this build's, outputs compared bit for bit; the bound on each ratio is 1 + twice the
                                   spread of the other build alternating with itself (hmm_fit_time.versus_parent)

python tools/vit_dur_time.py [--frames 1140000] [--shapes 40x256,40x1024,100x1024] [--repeats 4] [--parent-lib FILE] [--out FILE]"""
import argparse
import ctypes
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np

from hmm_fit_time import alternate, versus_parent
from units_time import cut

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DURATIONS = (1, 2, 3, 5, 8)


def sweep(new_fn, old_fn, outputs, repeats):
    """{S: the alternate() block of new_fn(S) against old_fn()}, the S = 1 block with outputs_bit_identical."""
    import torch
    out = {}
    for S in DURATIONS:
        blk = alternate(lambda: new_fn(S), old_fn, repeats)
        blk.update(first='new entry, min_duration %d' % S, second='old entry')
        if S == 1:
            new_fn(1)
            torch.cuda.synchronize()
            mine = [t.clone() for t in outputs]
            for t in outputs:
                t.fill_(-3)
            old_fn()
            torch.cuda.synchronize()
            blk['outputs_bit_identical'] = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(mine, outputs))
        out['S=%d' % S] = blk
    first = float(np.median(out['S=1']['first_ms']))
    out['new_over_old'] = {k: v['ratio_of_medians'] for k, v in out.items() if k.startswith('S=')}
    out['new_over_new_at_1'] = {k: round(float(np.median(v['first_ms'])) / first, 4) for k, v in out.items() if k.startswith('S=')}
    return out


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
    lw, ls, lr = (torch.from_numpy(t).cuda() for t in hmm.viterbi_tables(model.weights_, h.stay_))
    off_h, len_h = cut(T, D + K)
    off = torch.from_numpy(off_h).cuda()
    lens = torch.from_numpy(len_h.astype(np.int32)).cuda()
    lib = _lib.load()
    p = _lib.ptr
    n_utt, max_len = len(len_h), int(len_h.max())
    ws = torch.empty(int(lib.abn_hmm_viterbi_ws_bytes(n_utt, max_len, K, D)), dtype=torch.uint8, device='cuda')
    ids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    lp = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    nsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    ng = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    res = {'T': T, 'D': D, 'K': K, 'stay': float(np.float32(a.stay)), 'penalty': a.penalty, 'utterances': n_utt, 'max_len': max_len}

    def hargs(out):
        return (p(table), T, D, p(off), p(lens), n_utt, p(shift), p(A), p(B), p(c0), p(lw), p(ls), p(lr), K, p(out), p(lp), p(nsw),
                p(ng), p(ws), ws.numel(), _lib.stream())

    def vit(which=lib, out=ids):
        _lib.check(which.abn_hmm_viterbi(*hargs(out)), 'abn_hmm_viterbi')

    def vit_dur(S):
        _lib.check(lib.abnx_hmm_viterbi_dur(*(hargs(ids) + (S,))), 'abnx_hmm_viterbi_dur')

    ktable, kshift, good = kmeans.prepare(table, 'euclidean')
    kst = kmeans.LloydState(kmeans.initial_centroids(ktable, kshift, good, K, 0), T, table.device)
    for _ in range(3):
        kmeans.lloyd_iteration(ktable, kshift, kst)
    kws = torch.empty(int(lib.abn_kmeans_viterbi_ws_bytes(n_utt, max_len, K, D)), dtype=torch.uint8, device='cuda')
    kids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
    kobj = torch.zeros(n_utt, dtype=torch.float64, device='cuda')
    knsw = torch.zeros(n_utt, dtype=torch.int32, device='cuda')
    pen = float(np.float32(a.penalty / 2.0))

    def kargs(out):
        return (p(ktable), T, D, p(off), p(lens), n_utt, p(kshift), p(kst.m), p(kst.b), K, pen, p(out), p(kobj), p(knsw), p(kws),
                kws.numel(), _lib.stream())

    def kvit(which=lib, out=kids):
        _lib.check(which.abn_kmeans_viterbi(*kargs(out)), 'abn_kmeans_viterbi')

    def kvit_dur(S):
        _lib.check(lib.abnx_kmeans_viterbi_dur(*(kargs(kids) + (S,))), 'abnx_kmeans_viterbi_dur')

    vit(), kvit(), vit_dur(8), kvit_dur(8)
    res['abnx_hmm_viterbi_dur'] = sweep(vit_dur, vit, (ids, lp, nsw, ng), a.repeats)
    switches = {}
    for S in DURATIONS:
        vit_dur(S)
        switches['S=%d' % S] = int(nsw.sum())
    res['abnx_hmm_viterbi_dur']['switches'] = switches
    res['abnx_kmeans_viterbi_dur'] = sweep(kvit_dur, kvit, (kids, kobj, knsw), a.repeats)
    switches = {}
    for S in DURATIONS:
        kvit_dur(S)
        switches['S=%d' % S] = int(knsw.sum())
    res['abnx_kmeans_viterbi_dur']['switches'] = switches

    if parent is not None:
        def same(fn, out, other, rest):
            fn()
            torch.cuda.synchronize()
            mine = [t.clone() for t in rest]
            fn(parent, other)
            torch.cuda.synchronize()
            return torch.equal(out, other) and all(torch.equal(m.view(torch.uint8), t.view(torch.uint8)) for m, t in zip(mine, rest))

        oids = torch.full((T,), -1, dtype=torch.int32, device='cuda')
        res['abn_hmm_viterbi_vs_parent_build'] = versus_parent(vit, lambda: vit(parent, oids), lambda: same(vit, ids, oids, (lp, nsw, ng)))
        res['abn_kmeans_viterbi_vs_parent_build'] = versus_parent(kvit, lambda: kvit(parent, oids),
                                                                  lambda: same(kvit, kids, oids, (kobj, knsw)))
    for name in ('abnx_hmm_viterbi_dur', 'abnx_kmeans_viterbi_dur'):
        print('D = %d, K = %d: %s new / old %s, time against S %s' % (D, K, name, res[name]['new_over_old'], res[name]['new_over_new_at_1']),
              file=sys.stderr, flush=True)
    torch.cuda.empty_cache()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument('--frames', type=int, default=1140000)
    ap.add_argument('--shapes', default='40x256,40x1024,100x1024', help='D x K of the workloads')
    ap.add_argument('--stay', type=float, default=0.9)
    ap.add_argument('--penalty', type=float, default=6.0, help='the k-means decoder\'s penalty (units of the distortion)')
    ap.add_argument('--repeats', type=int, default=4, help='medians per route of an alternating pair')
    ap.add_argument('--parent-lib', default=None, metavar='FILE', help='the parent commit\'s libabnet3_hip.so')
    ap.add_argument('--out', default=os.path.join(ROOT, 'profiles', 'vit_dur_time.json'))
    a = ap.parse_args()
    import torch
    from abnet3_amd import _lib
    parent = None
    if a.parent_lib:
        lib = _lib.load()
        parent = ctypes.CDLL(os.path.abspath(a.parent_lib))
        for name in ('abn_hmm_viterbi', 'abn_kmeans_viterbi'):
            fn, own = getattr(parent, name), getattr(lib, name)
            fn.restype, fn.argtypes = own.restype, own.argtypes
    shapes = [tuple(int(v) for v in s.split('x')) for s in a.shapes.split(',')]
    res = {'device': torch.cuda.get_device_name(0), 'calls_per_median': 15, 'medians_per_route': a.repeats,
           'protocol': 'settle 0.3 s of untimed calls, then the median of 15 device-event timings per route; alternating routes '
                       'take `medians_per_route` medians each in one process',
           'workloads': [workload(a.frames, D, K, a, parent) for D, K in shapes]}
    print(json.dumps(res))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, 'w') as fh:
            fh.write(json.dumps(res, indent=1) + '\n')
    for wl in res['workloads']:
        for key, block in wl.items():
            if key.endswith('_vs_parent_build'):
                assert block['outputs_bit_identical'], key
            if key.startswith('abnx_'):
                assert block['S=1']['outputs_bit_identical'], key


if __name__ == '__main__':
    main()
